// The variational bound of lda-c's `lda est` (the number it writes to likelihood.dat) and the α
// sufficient statistic, from the E-step's γ and the doc-major (document, word, count) pairs: the
// one device reduction behind VarLDA's convergence exit and α estimation (ops.vem_bound;
// oni355/ref/vem_spec.py `bound` is the specification). Everything is f64, from f32 inputs.
//
//     S_d  = Σ_{k<K} γ_dk        E_dk = ψ(γ_dk) − ψ(S_d)        x_dk = exp(E_dk), 0 past K
//     A_d  = Σ_{k<K} ψ(γ_dk) − K·ψ(S_d)
//     T_d  = lgamma(Kα) − K·lgamma(α) − lgamma(S_d) + Σ_{k<K} [ (α − γ_dk)·E_dk + lgamma(γ_dk) ]
//     s_p  = Σ_{k<K} f64(table[w_p,k]) · x_{d_p,k}                        (ascending k)
//     L_d  = T_d + Σ_{p in d} c_p · log(s_p)          tot = (Σ_d L_d, Σ_d A_d)
//
// The pair term is lda-c's Σ_k φ_pk(E_k − log φ_pk + log β_kw) at the optimal φ_pk = table·x / s,
// where it collapses to log s_p: no [P, K] responsibilities are formed. E ≤ 0, so x needs no max
// shift in f64 (ψ(0.01) − ψ(S) ≥ −114: exp of it is a normal number).
//
// k_vbound_rows   a group of G = next-pow2(KS) lanes (the whole wave from KS = 33, then KQ = ⌈KS/64⌉
//                 columns a lane: ONI_VEM_SHAPES of vem.hip) owns a γ row: ψ and lgamma of its
//                 columns, the row sums S and Σψ by a fixed xor butterfly inside the group (an xor
//                 butterfly of commutative adds leaves the same bits in every lane), ψ(S) and
//                 lgamma(S) on the group's first lane only and broadcast, then E, x and the sum of
//                 (α − γ)E + lgamma γ by a second butterfly. Writes x f64 [D][KS], T_d and A_d.
//                 lgamma(Kα) − K·lgamma(α) is one number per launch and comes from the host.
// k_vbound_pairs  lane = doc-major pair, pair i on lane i mod 64 of wave ⌊i/64⌋ whatever the grid.
//                 Neighbouring lanes share a document, so its x row (8·KS bytes) comes from cache for
//                 most of them; the table row is read as 16-byte loads and widened; x as 16-byte
//                 double pairs. c·log(s) with the log in f64, then a segmented inclusive scan keyed
//                 by pair_doc (six __shfl_up steps). A segment strictly inside the wave is a whole
//                 document's pair sum and is written to doc[d]; one touching lane 0 is the wave's
//                 HEAD, one touching only lane 63 its TAIL: slots 2w and 2w + 1 of a scratch buffer
//                 nobody initialises. As in fit.hip and vem.hip the slot of a document's part in a
//                 wave follows from the document's pair range alone; a slot not written is not read.
//                 A pair with a word outside the table keeps its document's segment whole and adds 0.
// k_vbound_docs   lane = document, tiles of 256 documents. The pair range comes from doc_pair_ptr
//                 (clamped to [0, P]), so nothing is searched. The wave records are added in wave
//                 order: up to kLightWaves by the lane itself; more (a flow IP with 10^5 pairs is
//                 1600 records) by the whole wave, one such document after the other, lane-strided
//                 compensated sums and a fixed xor butterfly. L_d = T_d + pair sum is written, and
//                 the tile's ΣL and ΣA go through a wave butterfly, LDS and thread 0 in wave order.
// k_vbound_total  one wave adds the ⌈D/256⌉ tile partials (lane-strided, compensated, butterfly).
//
// Deviation from the sketch: none in the split. The α-only constant is computed once on the host
// instead of once per row, and the document pass reuses doc[d] as the hand-over of a document whose
// pairs lie strictly inside one wave (fit.hip does the same), so there is no [D] pair-sum buffer.
//
// Which values are added, and in what order, follows from pair index, document id and tile index
// only: no atomics, the same bits whatever the grid and from run to run. The only barriers are the
// two of k_vbound_docs, inside a grid-stride loop over tiles whose trip count is block-uniform;
// nothing returns before them.
//
// No MFMA: s_p is a per-document matrix-vector product over gathered table rows. Vector loads and
// stores only, no inline assembly. There is no f32 arithmetic here beyond widening loads, so the
// file needs none of the per-file build flags of fit.hip / vfold.hip / vem.hip.
//
// Pairs naming a document outside [0, D) or a word outside [0, rows) contribute nothing and nothing
// is read or written through them.
#include <math.h>

#include "oni_common.h"

namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / oni::kWave;
constexpr int kLightWaves = 8;  // records a document's own lane still adds itself

// ψ(x), x > 0, in f64: the recurrence two steps a division, 1/x + 1/(x + 1) = (2x + 1)/(x(x + 1)),
// up to x ≥ 10, then the asymptotic series through B14 (the next term is below 5e-17 there). The
// shift is a bounded loop, so no input (NaN, ≤ 0) can spin.
__device__ __forceinline__ double digamma_f64(double x) {
  double acc = 0.0;
#pragma unroll 1
  for (int i = 0; i < 5; ++i) {
    if (x < 10.0) {
      acc += (2.0 * x + 1.0) / (x * (x + 1.0));
      x += 2.0;
    }
  }
  const double inv = 1.0 / x, f = inv * inv;
  const double ser =
      f * (1.0 / 12 - f * (1.0 / 120 - f * (1.0 / 252 - f * (1.0 / 240 - f * (1.0 / 132 - f * (691.0 / 32760 - f * (1.0 / 12)))))));
  return ((log(x) - 0.5 * inv) - ser) - acc;
}

template <int G, int KQ>
__global__ __launch_bounds__(kBlock) void k_vbound_rows(const float* __restrict__ gamma, int64_t D, int KS, int K,
                                                        double alpha, double c0, double* __restrict__ x,
                                                        double* __restrict__ T, double* __restrict__ A) {
  constexpr int NSUB = oni::kWave / G;
  const int lane = threadIdx.x & (oni::kWave - 1), wave = threadIdx.x / oni::kWave;
  const int sg = lane / G, k0 = lane % G;
  for (int64_t base = ((int64_t)blockIdx.x * kWaves + wave) * NSUB; base < D;
       base += (int64_t)gridDim.x * kWaves * NSUB) {  // wave-uniform trip count
    const int64_t d = base + sg;
    const bool live = d < D;
    double g[KQ], psi[KQ], lg[KQ];
    double S = 0.0, sp = 0.0;
#pragma unroll
    for (int kk = 0; kk < KQ; ++kk) {
      const int k = k0 + kk * oni::kWave;
      g[kk] = psi[kk] = lg[kk] = 0.0;
      if (live && k < K) {
        g[kk] = (double)gamma[d * KS + k];
        psi[kk] = digamma_f64(g[kk]);
        lg[kk] = lgamma(g[kk]);
      }
      S += g[kk];
      sp += psi[kk];
    }
#pragma unroll
    for (int m = 1; m < G; m <<= 1) {
      S += __shfl_xor(S, m);
      sp += __shfl_xor(sp, m);
    }
    double pS = 0.0, lS = 0.0;
    if (live && k0 == 0) {  // once per row
      pS = digamma_f64(S);
      lS = lgamma(S);
    }
    pS = __shfl(pS, sg * G);
    lS = __shfl(lS, sg * G);
    double ts = 0.0;
#pragma unroll
    for (int kk = 0; kk < KQ; ++kk) {
      const int k = k0 + kk * oni::kWave;
      const bool on = live && k < K;
      const double E = psi[kk] - pS;
      if (on) ts += (alpha - g[kk]) * E + lg[kk];
      if (live && k < KS) x[d * KS + k] = on ? exp(E) : 0.0;
    }
#pragma unroll
    for (int m = 1; m < G; m <<= 1) ts += __shfl_xor(ts, m);
    if (live && k0 == 0) {
      T[d] = (c0 - lS) + ts;
      A[d] = sp - (double)K * pS;
    }
  }
}

// Σ_k f64(t[k]) · x[k] in ascending k: 16-byte loads on both sides
template <int KS>
__device__ __forceinline__ double dot_tx(const float* __restrict__ t, const double* __restrict__ x, int ks) {
  double s = 0.0;
  const int n = KS > 0 ? KS : ks;
#pragma unroll
  for (int j = 0; j < n; j += 4) {
    const float4 a = *reinterpret_cast<const float4*>(t + j);
    const double2 b0 = *reinterpret_cast<const double2*>(x + j);
    const double2 b1 = *reinterpret_cast<const double2*>(x + j + 2);
    s = s + (double)a.x * b0.x;
    s = s + (double)a.y * b0.y;
    s = s + (double)a.z * b1.x;
    s = s + (double)a.w * b1.y;
  }
  return s;
}

template <int KS>
__global__ __launch_bounds__(kBlock) void k_vbound_pairs(const double* __restrict__ x, const float* __restrict__ table,
                                                         int ks_dyn, const int32_t* __restrict__ pdoc,
                                                         const int32_t* __restrict__ pword,
                                                         const int32_t* __restrict__ pcnt, int64_t P, int32_t D,
                                                         int32_t rows, double* __restrict__ doc_sum,
                                                         double* __restrict__ wrec) {
  const int ks = KS > 0 ? KS : ks_dyn;
  const int lane = threadIdx.x & (oni::kWave - 1);
  for (int64_t base = (int64_t)blockIdx.x * kBlock; base < P; base += (int64_t)gridDim.x * kBlock) {
    const int64_t i = base + threadIdx.x;
    if (i - lane >= P) continue;  // a wave past the end (wave-uniform; no block barrier in this kernel)
    int doc = -1;
    double a = 0.0;
    if (i < P) {
      const int32_t d = pdoc[i], w = pword[i];
      if ((uint32_t)d < (uint32_t)D) {
        doc = d;
        if ((uint32_t)w < (uint32_t)rows) {
          const double s = dot_tx<KS>(table + (int64_t)w * ks, x + (int64_t)d * ks, ks);
          a = (double)pcnt[i] * log(s);
        }
      }
    }
    // segmented inclusive scan in lane order: pair_doc is non-decreasing, so equal keys d lanes
    // apart mean one segment in between
#pragma unroll
    for (int d = 1; d < oni::kWave; d <<= 1) {
      const int od = __shfl_up(doc, d);
      const double o = __shfl_up(a, d);
      if (lane >= d && od == doc) a = o + a;
    }
    const int prev = __shfl_up(doc, 1), next = __shfl_down(doc, 1);
    const bool first = lane == 0 || prev != doc;
    const bool last = lane == oni::kWave - 1 || next != doc;
    const uint64_t firsts = __ballot(first);
    if (last && doc >= 0) {
      const int fl = 63 - __clzll((long long)(firsts & (~0ull >> (63 - lane))));  // the segment's first lane
      if (fl != 0 && lane != oni::kWave - 1) doc_sum[doc] = a;
      else wrec[2 * (i >> 6) + (fl != 0 ? 1 : 0)] = a;
    }
  }
}

// s += v with the rounding error collected in e (two-sum); once the sum is not finite (a −inf term)
// there is no error to collect, and inf − inf must not turn the sum into a NaN
__device__ __forceinline__ void comp_add(double& s, double& e, double v) {
  const double t = s + v;
  const double bb = t - s;
  const double err = (s - (t - bb)) + (v - bb);
  e += isfinite(t) ? err : 0.0;
  s = t;
}

__global__ __launch_bounds__(kBlock) void k_vbound_docs(const int64_t* __restrict__ dptr, int64_t P, int64_t D,
                                                        const double* __restrict__ T, const double* __restrict__ A,
                                                        const double* __restrict__ wrec, double* __restrict__ doc,
                                                        double* __restrict__ tpart) {
  __shared__ double s_l[kWaves], s_a[kWaves];
  const int lane = threadIdx.x & (oni::kWave - 1), wave = threadIdx.x / oni::kWave;
  for (int64_t base = (int64_t)blockIdx.x * kBlock; base < D; base += (int64_t)gridDim.x * kBlock) {  // block-uniform
    const int64_t d = base + threadIdx.x;
    double sum = 0.0;
    bool heavy = false;
    long long w0 = 0, w1 = -1;
    int slot0 = 0;  // the slot of the document's part in its first wave (head in every later wave)
    if (d < D) {
      int64_t lo = dptr[d], hi = dptr[d + 1];
      lo = lo < 0 ? 0 : (lo > P ? P : lo);
      hi = hi < lo ? lo : (hi > P ? P : hi);
      if (lo < hi) {
        w0 = lo >> 6;
        w1 = (hi - 1) >> 6;
        if (w0 == w1 && (lo & 63) != 0 && ((hi - 1) & 63) != 63) {
          sum = doc[d];  // k_vbound_pairs wrote the whole pair sum
        } else {
          slot0 = (lo & 63) != 0 ? 1 : 0;
          heavy = w1 - w0 >= kLightWaves;
          if (!heavy) {
            sum = wrec[2 * w0 + slot0];
            for (long long w = w0 + 1; w <= w1; ++w) sum += wrec[2 * w];
          }
        }
      }
    }
    // the wave's heavy documents, one after the other, by all of its lanes
    uint64_t todo = __ballot(heavy);
    while (todo) {
      const int src = __ffsll((unsigned long long)todo) - 1;
      todo &= todo - 1;
      const long long h0 = __shfl(w0, src), h1 = __shfl(w1, src);
      const int hs = __shfl(slot0, src);
      double v = 0.0, e = 0.0;
      for (long long w = h0 + lane; w <= h1; w += oni::kWave) comp_add(v, e, wrec[2 * w + (w == h0 ? hs : 0)]);
      v = v + e;
#pragma unroll
      for (int m = 1; m < oni::kWave; m <<= 1) v += __shfl_xor(v, m);
      if (lane == src) sum = v;
    }
    double l = 0.0, a = 0.0;
    if (d < D) {
      l = T[d] + sum;
      a = A[d];
      doc[d] = l;
    }
    // the tile's partial totals, in a fixed order
#pragma unroll
    for (int m = 1; m < oni::kWave; m <<= 1) {
      l += __shfl_xor(l, m);
      a += __shfl_xor(a, m);
    }
    if (lane == 0) {
      s_l[wave] = l;
      s_a[wave] = a;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      double y = s_l[0], z = s_a[0];
      for (int w = 1; w < kWaves; ++w) {
        y += s_l[w];
        z += s_a[w];
      }
      const int64_t tile = base / kBlock;
      tpart[2 * tile] = y;
      tpart[2 * tile + 1] = z;
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(oni::kWave) void k_vbound_total(const double* __restrict__ tpart, int64_t nT,
                                                             double* __restrict__ tot) {
  const int lane = threadIdx.x;
  double y = 0.0, ey = 0.0, z = 0.0, ez = 0.0;
  for (int64_t t = lane; t < nT; t += oni::kWave) {
    comp_add(y, ey, tpart[2 * t]);
    comp_add(z, ez, tpart[2 * t + 1]);
  }
  y = y + ey;
  z = z + ez;
#pragma unroll
  for (int m = 1; m < oni::kWave; m <<= 1) {
    y += __shfl_xor(y, m);
    z += __shfl_xor(z, m);
  }
  if (lane == 0) {
    tot[0] = y;
    tot[1] = z;
  }
}

}  // namespace

// the lane-group ladder of vem.hip (kept as a copy so that file stays as it is)
#define ONI_VBOUND_SHAPES(KS_, CALL)     \
  if (KS_ <= 4) { CALL(4, 1) }           \
  else if (KS_ <= 8) { CALL(8, 1) }      \
  else if (KS_ <= 16) { CALL(16, 1) }    \
  else if (KS_ <= 32) { CALL(32, 1) }    \
  else if (KS_ <= 64) { CALL(64, 1) }    \
  else if (KS_ <= 128) { CALL(64, 2) }   \
  else { CALL(64, 4) }

// gamma f32 [D][KS], table f32 [rows][KS], doc-major pdoc (non-decreasing) / pword / pcnt int32 [P],
// doc_pair_ptr int64 [D + 1]: doc_out f64 [D] = L_d, tot_out f64 [2] = Σ L_d, Σ A_d.
// scratch: D·KS + 2·D + 2·⌈P/64⌉ + 2·⌈D/256⌉ doubles (scratch_len says how many there are),
// uninitialised. grid: blocks of every pass (0: sized from P and D); the result does not depend on it.
ONI_API int oni_vem_bound(const float* gamma, const float* table, int64_t rows, int KS, int K, const int32_t* pdoc,
                          const int32_t* pword, const int32_t* pcnt, const int64_t* doc_pair_ptr, int64_t P, int64_t D,
                          double alpha, double* doc_out, double* tot_out, double* scratch, int64_t scratch_len, int grid,
                          hipStream_t s) {
  if (K < 1 || K > KS || KS % 4 != 0 || KS > 256 || P < 0 || D < 0 || D > 0x7FFFFFFFll || rows < 1 ||
      rows > 0x7FFFFFFFll || !(alpha > 0.0) || grid < 0 || grid > 65535 || tot_out == nullptr || scratch == nullptr)
    return (int)hipErrorInvalidValue;
  if (D > 0 && (gamma == nullptr || doc_out == nullptr || doc_pair_ptr == nullptr)) return (int)hipErrorInvalidValue;
  if (P > 0 && (table == nullptr || pdoc == nullptr || pword == nullptr || pcnt == nullptr || D == 0))
    return (int)hipErrorInvalidValue;
  const int64_t nW = (P + oni::kWave - 1) / oni::kWave, nT = (D + kBlock - 1) / kBlock;
  if (scratch_len < D * KS + 2 * D + 2 * nW + 2 * nT) return (int)hipErrorInvalidValue;
  double* x = scratch;
  double* T = x + D * KS;
  double* A = T + D;
  double* wrec = A + D;
  double* tpart = wrec + 2 * nW;
  const double c0 = lgamma((double)K * alpha) - (double)K * lgamma(alpha);
  if (D > 0) {
#define ONI_R(G_, KQ_)                                                                                              \
  k_vbound_rows<G_, KQ_><<<grid > 0 ? (unsigned)grid : oni::grid_for((D + 64 / G_ - 1) / (64 / G_), kWaves, 4096), \
                           kBlock, 0, s>>>(gamma, D, KS, K, alpha, c0, x, T, A);
    ONI_VBOUND_SHAPES(KS, ONI_R)
#undef ONI_R
  }
  if (P > 0) {
    const unsigned g = grid > 0 ? (unsigned)grid : oni::grid_for(P, kBlock, 4096);
    const int32_t Di = (int32_t)D, Ri = (int32_t)rows;
#define ONI_P(k_) \
  if (KS == k_) k_vbound_pairs<k_><<<g, kBlock, 0, s>>>(x, table, KS, pdoc, pword, pcnt, P, Di, Ri, doc_out, wrec); else
    ONI_P(20) ONI_P(56) ONI_P(100)
#undef ONI_P
    k_vbound_pairs<0><<<g, kBlock, 0, s>>>(x, table, KS, pdoc, pword, pcnt, P, Di, Ri, doc_out, wrec);
  }
  if (D > 0)
    k_vbound_docs<<<grid > 0 ? (unsigned)grid : oni::grid_for(D, kBlock, 2048), kBlock, 0, s>>>(doc_pair_ptr, P, D, T, A,
                                                                                              wrec, doc_out, tpart);
  k_vbound_total<<<1, oni::kWave, 0, s>>>(tpart, nT, tot_out);
  return (int)hipGetLastError();
}
