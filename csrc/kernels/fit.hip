// oni355 -- how well a saved model fits a scored batch, per document (IP) and in total.
//
//   ll_d = Σ_{pairs (d,w)} c_dw · log( Σ_k θ_dk · φ_wk )
//
// over the doc-major list of distinct (doc, word, count) pairs the pipeline already holds after
// fold-in, together with the document's tokens (Σ c), its out-of-vocabulary tokens (Σ c over the
// table's row `oov_id`) and its smallest pair score. The pair score is oni::dot_rows, the dot of
// k_pair_score (f32, fixed k order, 16-B loads, no contraction), so `min_score` is bitwise the
// minimum of ops.pair_score over the document; the term is f64(c) · log(f64(score)), the log in
// f64. A score of exactly 0 gives -inf, which propagates into the document and the total.
//
// Every value is a pure function of the inputs: which values are added to which, and in what
// order, depends on a pair's index and a document's id only, never on the grid, and there are no
// floating-point atomics (no atomics at all). Same inputs, same bits, whatever grid is launched.
//
// k_fit_pairs -- one lane per pair; pair i belongs to lane i % 64 of wave ⌊i/64⌋ whatever the grid.
//   Doc-major order means neighbouring lanes read the same θ row (one request per wave and row
//   piece). The wave runs a segmented inclusive scan keyed by pair_doc over (f64 ll, i64 tokens,
//   i64 oov tokens, f32 min) in registers (six __shfl_up steps, each a fixed lane distance), after
//   which the last lane of every segment holds the segment's values.
//     * a segment strictly inside the wave is a whole document: its last lane writes the result;
//     * a segment touching lane 0 is the wave's HEAD partial, one touching lane 63 only its TAIL
//       partial: written to the wave's record in the scratch buffer (slots 2w and 2w + 1).
//   Which slot holds a document's part in a wave follows from the document's pair range alone, so
//   the records carry no doc ids and need no initialisation: a slot that was not written is not read.
// k_fit_docs -- one lane per document; document d belongs to lane d % 256 of tile ⌊d/256⌋.
//   The lane finds its pair range [lo, hi) by a lower bound on pair_doc (neighbouring lanes walk
//   neighbouring paths: the upper levels are one cache line for the wave) and a short gallop from
//   lo for hi (a typical IP has ~7 pairs). No pairs: zeros and +inf. Written by k_fit_pairs: read
//   back for the totals. Else the document's wave partials are combined in wave order:
//     * up to kHeavyWaves waves by the lane itself;
//     * more (an IP with 10^5..10^6 pairs is 10^3..10^4 waves) by the whole wave, one such document
//       after the other: lane-strided sums, then the xor butterfly of k_tail_final. The lane sums
//       are compensated (two-sum), so the error of a 10^4-term lane sum stays that of one addition
//       and the tolerance derived for a pairwise sum holds for heavy documents too.
//   Light and heavy documents share this one path; nothing loops on the host.
//   The block then reduces its tile's 256 documents in a fixed order (wave butterfly, four waves in
//   LDS, thread 0 adds them in wave order) into the tile's partial totals.
// k_fit_total -- one wave adds the ⌈D/256⌉ tile partials (lane-strided, compensated, butterfly).
//
// Deviation from "one single block over the D document values" for the totals: a single block
// streaming 24 B for each of 367k documents is bound by one CU's memory path (~9 MB through one
// CU), several times the cost of the rest; the tile partials cost k_fit_docs one LDS round and
// leave the single block 1436 records. The order is as fixed as before: tiles are defined by D.
//
// Pairs naming a document outside [0, D) or a word outside [0, oov_id] are skipped (nothing is
// read or written through them). Vector loads and stores only, no inline assembly.
#include "oni_common.h"

namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / oni::kWave;
constexpr int kHeavyWaves = 8;  // a document over more waves than this is combined by a whole wave

struct Acc {
  double ll;
  long long tok, oov;
  float mn;
};

__device__ __forceinline__ Acc acc_zero() { return Acc{0.0, 0ll, 0ll, __builtin_inff()}; }

// a's pairs come before b's
__device__ __forceinline__ Acc acc_join(const Acc& a, const Acc& b) {
  return Acc{a.ll + b.ll, a.tok + b.tok, a.oov + b.oov, b.mn < a.mn ? b.mn : a.mn};
}

__device__ __forceinline__ Acc acc_shfl_up(const Acc& a, int d) {
  return Acc{__shfl_up(a.ll, d), __shfl_up(a.tok, d), __shfl_up(a.oov, d), __shfl_up(a.mn, d)};
}

__device__ __forceinline__ Acc acc_shfl_xor(const Acc& a, int m) {
  return Acc{__shfl_xor(a.ll, m), __shfl_xor(a.tok, m), __shfl_xor(a.oov, m), __shfl_xor(a.mn, m)};
}

// s += x with the rounding error collected in e (Knuth's two-sum); once the sum is not finite
// (a -inf term) there is no error to collect, and inf - inf must not turn the sum into a NaN
__device__ __forceinline__ void comp_add(double& s, double& e, double x) {
  const double t = s + x;
  const double bb = t - s;
  const double err = (s - (t - bb)) + (x - bb);
  e += isfinite(t) ? err : 0.0;
  s = t;
}

// the wave records and the tile partials, carved out of one scratch buffer of 8-byte words
struct Scratch {
  double* w_ll;      // [2·nW] head / tail partial of every wave
  long long* w_tok;  // [2·nW]
  long long* w_oov;  // [2·nW]
  float* w_min;      // [2·nW]
  double* t_ll;      // [nT] tile partials
  long long* t_tok;  // [nT]
  long long* t_oov;  // [nT]
  long long* t_docs; // [nT] documents with at least one token
};

__host__ __device__ inline int64_t n_waves(int64_t P) { return (P + oni::kWave - 1) / oni::kWave; }
__host__ __device__ inline int64_t n_tiles(int64_t D) { return (D + kBlock - 1) / kBlock; }

template <int KS>
__global__ __launch_bounds__(kBlock) void k_fit_pairs(const float* __restrict__ theta, const float* __restrict__ table,
                                                      int ks_dyn, const int32_t* __restrict__ pdoc,
                                                      const int32_t* __restrict__ pword,
                                                      const int32_t* __restrict__ pcnt, int64_t P, int32_t D,
                                                      int32_t oov_id, double* __restrict__ ll,
                                                      long long* __restrict__ tok, long long* __restrict__ oov,
                                                      float* __restrict__ mn, Scratch sc) {
  const int ks = KS > 0 ? KS : ks_dyn;
  const int lane = threadIdx.x & (oni::kWave - 1);
  for (int64_t base = (int64_t)blockIdx.x * kBlock; base < P; base += (int64_t)gridDim.x * kBlock) {
    const int64_t i = base + threadIdx.x;
    if (i - lane >= P) continue;  // a wave past the end (wave-uniform)
    int doc = -1;
    Acc a = acc_zero();
    if (i < P) {
      const int32_t d = pdoc[i], w = pword[i];
      if ((uint32_t)d < (uint32_t)D && (uint32_t)w <= (uint32_t)oov_id) {
        const float* t = theta + (int64_t)d * ks;
        const float* f = table + (int64_t)w * ks;
        const float s = KS > 0 ? oni::dot_rows<(KS > 0 ? KS : 4)>(t, f) : oni::dot_rows_dyn(t, f, ks);
        const long long c = pcnt[i];
        doc = d;
        a = Acc{(double)c * log((double)s), c, w == oov_id ? c : 0ll, s};
      }
    }
    // segmented inclusive scan in lane order: pair_doc is non-decreasing, so equal keys d lanes
    // apart mean one segment in between
#pragma unroll
    for (int d = 1; d < oni::kWave; d <<= 1) {
      const int od = __shfl_up(doc, d);
      const Acc o = acc_shfl_up(a, d);
      if (lane >= d && od == doc) a = acc_join(o, a);
    }
    const int prev = __shfl_up(doc, 1), next = __shfl_down(doc, 1);
    const bool first = lane == 0 || prev != doc;
    const bool last = lane == oni::kWave - 1 || next != doc;
    const uint64_t firsts = __ballot(first);
    if (last && doc >= 0) {
      // the segment's first lane: the highest `first` bit at or below this lane
      const int fl = 63 - __clzll((long long)(firsts & (~0ull >> (63 - lane))));
      if (fl != 0 && lane != oni::kWave - 1) {
        ll[doc] = a.ll;
        tok[doc] = a.tok;
        oov[doc] = a.oov;
        mn[doc] = a.mn;
      } else {
        const int64_t slot = 2 * (i >> 6) + (fl != 0 ? 1 : 0);
        sc.w_ll[slot] = a.ll;
        sc.w_tok[slot] = a.tok;
        sc.w_oov[slot] = a.oov;
        sc.w_min[slot] = a.mn;
      }
    }
  }
}

// first index in [lo, P) whose pair_doc is >= d
__device__ __forceinline__ int64_t lower_bound(const int32_t* __restrict__ pdoc, int64_t lo, int64_t hi, int64_t d) {
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if ((int64_t)pdoc[mid] < d) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

__device__ __forceinline__ Acc load_slot(const Scratch& sc, int64_t slot) {
  return Acc{sc.w_ll[slot], sc.w_tok[slot], sc.w_oov[slot], sc.w_min[slot]};
}

__global__ __launch_bounds__(kBlock) void k_fit_docs(const int32_t* __restrict__ pdoc, int64_t P, int64_t D,
                                                     double* __restrict__ ll, long long* __restrict__ tok,
                                                     long long* __restrict__ oov, float* __restrict__ mn,
                                                     Scratch sc) {
  __shared__ double s_ll[kWaves];
  __shared__ long long s_tok[kWaves], s_oov[kWaves], s_docs[kWaves];
  const int lane = threadIdx.x & (oni::kWave - 1), wave = threadIdx.x / oni::kWave;
  for (int64_t base = (int64_t)blockIdx.x * kBlock; base < D; base += (int64_t)gridDim.x * kBlock) {
    const int64_t d = base + threadIdx.x;
    Acc a = acc_zero();
    bool write = false, heavy = false;
    int64_t w0 = 0, w1 = -1;
    int slot0 = 0;  // the slot of the document's part in its first wave (head in every later wave)
    if (d < D) {
      const int64_t lo = lower_bound(pdoc, 0, P, d);
      int64_t step = 1, from = lo;  // gallop: hi is usually a few pairs past lo
      while (from + step < P && (int64_t)pdoc[from + step] <= d) {
        from += step;
        step <<= 1;
      }
      const int64_t hi = lower_bound(pdoc, from, from + step < P ? from + step : P, d + 1);
      if (lo == hi) {
        write = true;  // no pairs: zeros and +inf
      } else {
        w0 = lo >> 6;
        w1 = (hi - 1) >> 6;
        if (w0 == w1 && (lo & 63) != 0 && ((hi - 1) & 63) != 63) {
          a = Acc{ll[d], tok[d], oov[d], 0.f};  // k_fit_pairs wrote the document (min is not totalled)
        } else {
          write = true;
          slot0 = (lo & 63) != 0 ? 1 : 0;
          heavy = w1 - w0 >= kHeavyWaves;
          if (!heavy) {
            a = load_slot(sc, 2 * w0 + slot0);
            for (int64_t w = w0 + 1; w <= w1; ++w) a = acc_join(a, load_slot(sc, 2 * w));
          }
        }
      }
    }
    // the wave's heavy documents, one after the other, by all of its lanes
    uint64_t todo = __ballot(heavy);
    while (todo) {
      const int src = __ffsll((unsigned long long)todo) - 1;
      todo &= todo - 1;
      const int64_t hw0 = __shfl((long long)w0, src), hw1 = __shfl((long long)w1, src);
      const int hs = __shfl(slot0, src);
      Acc v = acc_zero();
      double e = 0.0;
      for (int64_t w = hw0 + lane; w <= hw1; w += oni::kWave) {
        const Acc p = load_slot(sc, 2 * w + (w == hw0 ? hs : 0));
        comp_add(v.ll, e, p.ll);
        v.tok += p.tok;
        v.oov += p.oov;
        v.mn = p.mn < v.mn ? p.mn : v.mn;
      }
      v.ll = v.ll + e;
#pragma unroll
      for (int m = 1; m < oni::kWave; m <<= 1) v = acc_join(v, acc_shfl_xor(v, m));
      if (lane == src) a = v;
    }
    if (write) {
      ll[d] = a.ll;
      tok[d] = a.tok;
      oov[d] = a.oov;
      mn[d] = a.mn;
    }
    // the tile's partial totals, in a fixed order
    Acc t = Acc{a.ll, a.tok, a.oov, 0.f};
    long long docs = a.tok > 0 ? 1 : 0;
#pragma unroll
    for (int m = 1; m < oni::kWave; m <<= 1) {
      t = acc_join(t, acc_shfl_xor(t, m));
      docs += __shfl_xor(docs, m);
    }
    if (lane == 0) {
      s_ll[wave] = t.ll;
      s_tok[wave] = t.tok;
      s_oov[wave] = t.oov;
      s_docs[wave] = docs;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      double x = s_ll[0];
      long long y = s_tok[0], z = s_oov[0], n = s_docs[0];
      for (int w = 1; w < kWaves; ++w) {
        x += s_ll[w];
        y += s_tok[w];
        z += s_oov[w];
        n += s_docs[w];
      }
      const int64_t tile = base / kBlock;
      sc.t_ll[tile] = x;
      sc.t_tok[tile] = y;
      sc.t_oov[tile] = z;
      sc.t_docs[tile] = n;
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(oni::kWave) void k_fit_total(Scratch sc, int64_t nT, double* __restrict__ tot) {
  const int lane = threadIdx.x;
  double x = 0.0, e = 0.0;
  long long y = 0, z = 0, n = 0;
  for (int64_t t = lane; t < nT; t += oni::kWave) {
    comp_add(x, e, sc.t_ll[t]);
    y += sc.t_tok[t];
    z += sc.t_oov[t];
    n += sc.t_docs[t];
  }
  x = x + e;
#pragma unroll
  for (int m = 1; m < oni::kWave; m <<= 1) {
    x += __shfl_xor(x, m);
    y += __shfl_xor(y, m);
    z += __shfl_xor(z, m);
    n += __shfl_xor(n, m);
  }
  if (lane == 0) {
    tot[0] = x;
    tot[1] = (double)y;
    tot[2] = (double)z;
    tot[3] = (double)n;
  }
}

}  // namespace

// theta f32 [D][KS], table f32 [oov_id + 1][KS], pdoc (non-decreasing) / pword / pcnt int32 [P];
// ll f64 [D], tok / oov i64 [D], mn f32 [D], tot f64 [4] = Σ ll, Σ tokens, Σ oov tokens, documents
// with a token; scratch: 7·⌈P/64⌉ + 4·⌈D/256⌉ 8-byte words, uninitialised. grid: blocks of both
// passes (0: sized from P and D); the result does not depend on it.
ONI_API int oni_doc_fit(const float* theta, const float* table, int KS, const int32_t* pdoc, const int32_t* pword,
                        const int32_t* pcnt, int64_t P, int64_t D, int32_t oov_id, double* ll, long long* tok,
                        long long* oov, float* mn, double* tot, void* scratch, int grid, hipStream_t s) {
  if (KS < 4 || KS % 4 != 0 || P < 0 || D < 0 || D > 0x7FFFFFFFll || oov_id < 0 || grid < 0 || tot == nullptr ||
      scratch == nullptr)
    return (int)hipErrorInvalidValue;
  const int64_t nW = n_waves(P), nT = n_tiles(D);
  Scratch sc;
  long long* q = static_cast<long long*>(scratch);
  sc.w_ll = reinterpret_cast<double*>(q);
  sc.w_tok = q + 2 * nW;
  sc.w_oov = q + 4 * nW;
  sc.w_min = reinterpret_cast<float*>(q + 6 * nW);
  sc.t_ll = reinterpret_cast<double*>(q + 7 * nW);
  sc.t_tok = q + 7 * nW + nT;
  sc.t_oov = q + 7 * nW + 2 * nT;
  sc.t_docs = q + 7 * nW + 3 * nT;
  if (P > 0) {
    const unsigned g = grid > 0 ? (unsigned)grid : oni::grid_for(P, kBlock, 4096);
    const int32_t Di = (int32_t)D;
#define ONI_F(k_) \
  if (KS == k_) k_fit_pairs<k_><<<g, kBlock, 0, s>>>(theta, table, KS, pdoc, pword, pcnt, P, Di, oov_id, ll, tok, oov, mn, sc); else
    ONI_F(20) ONI_F(24) ONI_F(32) ONI_F(52) ONI_F(64) ONI_F(100) ONI_F(104) ONI_F(128)
#undef ONI_F
    k_fit_pairs<0><<<g, kBlock, 0, s>>>(theta, table, KS, pdoc, pword, pcnt, P, Di, oov_id, ll, tok, oov, mn, sc);
  }
  if (D > 0) {
    const unsigned g = grid > 0 ? (unsigned)grid : oni::grid_for(D, kBlock, 2048);
    k_fit_docs<<<g, kBlock, 0, s>>>(pdoc, P, D, ll, tok, oov, mn, sc);
  }
  k_fit_total<<<1, oni::kWave, 0, s>>>(sc, nT, tot);
  return (int)hipGetLastError();
}
