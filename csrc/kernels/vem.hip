// Variational EM (`lda est`, smoothed, fixed α and β): the M-step around k_vfold's E-step, over the
// distinct (document, word, count) pairs of the corpus. oni355/ref/vem_spec.py is the specification.
//
//     e_dk   = exp(ψ(γ_dk) − max_j ψ(γ_dj))                      k < K, 0 past K      k_vem_e
//     q_p    = c_p / Σ_k table[w_p,k] · e_{d_p,k}                                     k_vem_q
//     ss[w,k] = table[w,k] · Σ_{p : w_p = w} q_p · e_{d_p,k}                          k_vem_wsum, k_vem_wcomb
//     table[w,k] = (ss[w,k] + β) / (Σ_w ss[w,k] + Vβ), row V = β / (…)                k_vem_colpart, _coltot, _rows
//
// k_vem_e     a group of G = next-pow2(KS) lanes (64 from KS = 33, then KQ = ⌈KS/64⌉ values a lane)
//             owns a γ row: ψ, the row maximum by an xor butterfly inside the group, exp, zeros past K.
// k_vem_q     lane = doc-major pair: s_p is oni::dot_rows of the pair's table row and its document's
//             e row (neighbouring lanes share the e row), q_p is written straight to the pair's
//             word-major position (wm_pos), so the segmented sum below streams it.
// k_vem_wsum  the segmented sum of KS-wide e rows over the WORD-MAJOR pair list (built once per
//             model: stable sort by word, so a word's pairs keep ascending document order). Word
//             lengths are heavily skewed (head words own 10^5..10^6 pairs, most own a handful), so
//             the list is cut into index-aligned tiles of 64 pairs whatever the words are:
//               * a wave loads a tile with lane = pair (q, document, word: three coalesced reads),
//                 finds the word boundaries with ballots (wave-uniform) and walks each segment with
//                 lane broadcasts while lane = k gathers e[doc][k];
//               * for KS ≤ 32 the wave is 64/G groups of G lanes and each step takes 64/G pairs, one
//                 per group, so that a K = 20 model keeps 40 of 64 lanes busy instead of 20; the
//                 groups' sums are added in group order at the flush;
//               * four steps' gathers are issued before the first is consumed;
//               * a wave walks kRun = 4 consecutive tiles (a span of 256 pairs) and carries the open
//                 word's sums across them. A segment strictly inside the span is a finished word:
//                 multiplied by table[w,k], rounded to f32 and written. A segment touching the
//                 span's first pair is its HEAD partial, one touching only its last pair its TAIL
//                 partial: kept as f64 in the span's scratch record (slots 2·span and 2·span + 1).
//                 As in fit.hip the slot of a word's part in a span follows from the word's pair range
//                 alone, so records carry no ids and need no initialisation.
//               Records per span, not per tile, quarter the scratch buffer and the combine's reads
//               (a 10^6-pair word: 3907 records); 2.66M pairs are still 10^4 waves.
//             Sums are f64: a product of two f32 is exact in f64, the terms are non-negative and up
//             to 10^6 of them, and the kernel waits for row gathers (80..1024 B a pair), not for the
//             adds. One rounding to f32, at the multiply by φ.
// k_vem_wcomb a group of G lanes per word adds the word's span partials in span order: up to
//             kLight records by the group itself; more by the whole wave, one such word after the
//             other, groups striding over the records, then a fixed xor butterfly over the groups.
//             Words without pairs get zeros; words k_vem_wsum finished are left alone.
// k_vem_colpart / k_vem_coltot / k_vem_rows  column totals over V in f64 through partials of fixed
//             256-word tiles (row groups of a tile meet in LDS and are added in group order), a
//             final pass over the tiles in order, then the row pass writing the new table in f64
//             arithmetic rounded once, row V and the zero padding included.
//
// Every sum's order is fixed by pair index, word id and tile index alone: no atomics, the same bits
// whatever the grid. The only barriers are the two of k_vem_colpart, in a grid-stride loop over
// tiles whose trip count is block-uniform; nothing returns before them.
//
// No MFMA: inside a tile the useful work is one vector-matrix product per word (q over the word's
// pairs times their e rows), the words' lengths differ and the rows are gathered; a matrix
// instruction would multiply padding. No LDS staging of e rows either: each is read once per pair.
// Vector loads and stores only, no inline assembly.
//
// Pairs naming a document outside [0, D) or a word outside [0, V) contribute nothing and nothing is
// read or written through them.
#include "oni_common.h"

namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / oni::kWave;
constexpr int kRun = 4;                     // tiles a wave walks
constexpr int kSpan = kRun * oni::kWave;    // pairs of a scratch record
constexpr int kLight = 2;                   // records a word's own lane group still adds itself
constexpr int kAhead = 4;                   // steps whose gathers are in flight together
constexpr int kColTile = 256;               // words of a column partial

// ψ(x), x > 0: the series of k_vfold (vfold.hip), kept as a copy so that file stays as it is
__device__ __forceinline__ float digamma_f32(float x) {
  float acc = 0.f;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    if (x < 6.f) {
      acc += (2.f * x + 1.f) / (x * (x + 1.f));
      x += 2.f;
    }
  }
  const float inv = 1.f / x, inv2 = inv * inv;
  const float ser = inv2 * (0.083333333333f - inv2 * (0.0083333333333f - inv2 * (0.0039682539683f - inv2 * 0.0041666666667f)));
  return ((logf(x) - 0.5f * inv) - ser) - acc;
}

template <int G, int KQ>
__global__ __launch_bounds__(kBlock) void k_vem_e(const float* __restrict__ gamma, int64_t D, int KS, int K,
                                                  float* __restrict__ e) {
  constexpr int NSUB = oni::kWave / G;
  const int lane = threadIdx.x & (oni::kWave - 1), wave = threadIdx.x / oni::kWave;
  const int sg = lane / G, k0 = lane % G;
  for (int64_t base = ((int64_t)blockIdx.x * kWaves + wave) * NSUB; base < D;
       base += (int64_t)gridDim.x * kWaves * NSUB) {
    const int64_t d = base + sg;
    float psi[KQ];
    float m = -__builtin_inff();
#pragma unroll
    for (int kk = 0; kk < KQ; ++kk) {
      const int k = k0 + kk * oni::kWave;
      psi[kk] = -__builtin_inff();
      if (d < D && k < K) psi[kk] = digamma_f32(gamma[d * KS + k]);
      m = fmaxf(m, psi[kk]);
    }
#pragma unroll
    for (int x = 1; x < G; x <<= 1) m = fmaxf(m, __shfl_xor(m, x));
#pragma unroll
    for (int kk = 0; kk < KQ; ++kk) {
      const int k = k0 + kk * oni::kWave;
      if (d < D && k < KS) e[d * KS + k] = k < K ? expf(psi[kk] - m) : 0.f;
    }
  }
}

template <int KS>
__global__ __launch_bounds__(kBlock) void k_vem_q(const float* __restrict__ e, const float* __restrict__ table,
                                                  int ks_dyn, const int32_t* __restrict__ pdoc,
                                                  const int32_t* __restrict__ pword,
                                                  const int32_t* __restrict__ pcnt,
                                                  const int32_t* __restrict__ wm_pos, int64_t P, int32_t D,
                                                  int32_t rows, float* __restrict__ q) {
  const int ks = KS > 0 ? KS : ks_dyn;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < P; i += (int64_t)gridDim.x * kBlock) {
    const int32_t d = pdoc[i], w = pword[i];
    const int64_t o = wm_pos != nullptr ? (int64_t)wm_pos[i] : i;
    if ((uint64_t)o >= (uint64_t)P) continue;
    float v = 0.f;
    if ((uint32_t)d < (uint32_t)D && (uint32_t)w < (uint32_t)rows) {
      const float* a = table + (int64_t)w * ks;
      const float* b = e + (int64_t)d * ks;
      const float s = KS > 0 ? oni::dot_rows<(KS > 0 ? KS : 4)>(a, b) : oni::dot_rows_dyn(a, b, ks);
      v = (float)pcnt[i] / s;
    }
    q[o] = v;
  }
}

struct WsumArgs {
  const float* e;           // [D][KS]
  const float* q;           // [P] word-major
  const int32_t* wdoc;      // [P] word-major
  const int32_t* wword;     // [P] word-major, non-decreasing
  const float* table;       // [V + 1][KS]
  float* ss;                // [V][KS]
  double* scratch;          // [2·⌈P/kSpan⌉][KS]
  int64_t P;
  int32_t D, V, KS;
};

enum Flush { kWhole, kHead, kTail };

// the groups' sums in group order; group 0 then holds the segment's sums and writes them
template <int G, int KQ>
__device__ __forceinline__ void flush(const WsumArgs& a, int w, int64_t span, int how, int sg, int k0,
                                      const double (&acc)[KQ]) {
  constexpr int NSUB = oni::kWave / G;
#pragma unroll
  for (int kk = 0; kk < KQ; ++kk) {
    double tot = acc[kk];
    if (NSUB > 1) {
      tot = __shfl(acc[kk], k0);
#pragma unroll
      for (int s = 1; s < NSUB; ++s) tot += __shfl(acc[kk], s * G + k0);
    }
    const int k = k0 + kk * oni::kWave;
    if (sg == 0 && k < a.KS && (uint32_t)w < (uint32_t)a.V) {
      if (how == kWhole) a.ss[(int64_t)w * a.KS + k] = (float)((double)a.table[(int64_t)w * a.KS + k] * tot);
      else a.scratch[(2 * span + (how == kTail ? 1 : 0)) * a.KS + k] = tot;
    }
  }
}

template <int G, int KQ>
__global__ __launch_bounds__(kBlock) void k_vem_wsum(const WsumArgs a) {
  constexpr int NSUB = oni::kWave / G;
  const int lane = threadIdx.x & (oni::kWave - 1), wave = threadIdx.x / oni::kWave;
  const int sg = lane / G, k0 = lane % G;
  const int KS = a.KS;
  const int64_t nspan = (a.P + kSpan - 1) / kSpan;
  for (int64_t span = (int64_t)blockIdx.x * kWaves + wave; span < nspan; span += (int64_t)gridDim.x * kWaves) {
    double acc[KQ];
#pragma unroll
    for (int kk = 0; kk < KQ; ++kk) acc[kk] = 0.0;
    int curw = 0;
    bool open = false, head = false;  // a segment is open; it touches the span's first pair
    for (int t = 0; t < kRun; ++t) {
      const int64_t base = span * kSpan + (int64_t)t * oni::kWave;
      if (base >= a.P) break;  // wave-uniform
      const int nv = a.P - base < oni::kWave ? (int)(a.P - base) : oni::kWave;
      float qv = 0.f;
      int dv = -1, wv = -1;
      if (lane < nv) {
        qv = a.q[base + lane];
        dv = a.wdoc[base + lane];
        wv = a.wword[base + lane];
      }
      int s0 = 0;
      while (s0 < nv) {  // the tile's segments, wave-uniform
        const int w = __shfl(wv, s0);
        const unsigned long long other = __ballot(lane >= s0 && lane < nv && wv != w);
        const int s1 = other ? __ffsll(other) - 1 : nv;
        if (!open || w != curw) {
          if (open) flush<G, KQ>(a, curw, span, head ? kHead : kWhole, sg, k0, acc);
#pragma unroll
          for (int kk = 0; kk < KQ; ++kk) acc[kk] = 0.0;
          head = t == 0 && s0 == 0;
          open = true;
          curw = w;
        }
        for (int j = s0; j < s1; j += NSUB * kAhead) {
          float qq[kAhead], v[kAhead][KQ];
#pragma unroll
          for (int u = 0; u < kAhead; ++u) {
            const int p = j + u * NSUB + sg;
            const bool ok = p < s1;
            const int src = ok ? p : s0;
            const float qs = __shfl(qv, src);
            const int d = __shfl(dv, src);
            const bool live = ok && (uint32_t)d < (uint32_t)a.D;
            qq[u] = live ? qs : 0.f;
#pragma unroll
            for (int kk = 0; kk < KQ; ++kk) {
              const int k = k0 + kk * oni::kWave;
              v[u][kk] = live && k < KS ? a.e[(int64_t)d * KS + k] : 0.f;
            }
          }
#pragma unroll
          for (int u = 0; u < kAhead; ++u)
#pragma unroll
            for (int kk = 0; kk < KQ; ++kk) acc[kk] += (double)qq[u] * (double)v[u][kk];
        }
        s0 = s1;
      }
    }
    if (open) {
      const bool full = (span + 1) * kSpan <= a.P;  // the open segment touches the span's last pair
      flush<G, KQ>(a, curw, span, head ? kHead : (full ? kTail : kWhole), sg, k0, acc);
    }
  }
}

template <int G, int KQ>
__global__ __launch_bounds__(kBlock) void k_vem_wcomb(const int64_t* __restrict__ wptr, int64_t V, int KS,
                                                      const float* __restrict__ table,
                                                      const double* __restrict__ scratch, float* __restrict__ ss) {
  constexpr int NSUB = oni::kWave / G;
  const int lane = threadIdx.x & (oni::kWave - 1), wave = threadIdx.x / oni::kWave;
  const int sg = lane / G, k0 = lane % G;
  for (int64_t wb = ((int64_t)blockIdx.x * kWaves + wave) * NSUB; wb < V; wb += (int64_t)gridDim.x * kWaves * NSUB) {
    const int64_t w = wb + sg;
    long long r0 = 0, r1 = -1;
    int slot0 = 0;  // the slot of the word's part in its first span (head in every later one)
    bool write = false, heavy = false;
    double acc[KQ];
#pragma unroll
    for (int kk = 0; kk < KQ; ++kk) acc[kk] = 0.0;
    if (w < V) {
      const int64_t lo = wptr[w], hi = wptr[w + 1];
      if (lo >= hi) {
        write = true;  // no pairs: zeros
      } else {
        r0 = lo / kSpan;
        r1 = (hi - 1) / kSpan;
        if (!(r0 == r1 && lo % kSpan != 0 && (hi - 1) % kSpan != kSpan - 1)) {  // else k_vem_wsum wrote it
          write = true;
          slot0 = lo % kSpan != 0 ? 1 : 0;
          heavy = r1 - r0 >= kLight;
          if (!heavy) {
            for (long long r = r0; r <= r1; ++r) {
#pragma unroll
              for (int kk = 0; kk < KQ; ++kk) {
                const int k = k0 + kk * oni::kWave;
                if (k < KS) acc[kk] += scratch[(2 * r + (r == r0 ? slot0 : 0)) * KS + k];
              }
            }
          }
        }
      }
    }
    // the wave's heavy words, one after the other, by all of its groups
    unsigned long long todo = __ballot(heavy && k0 == 0);
    while (todo) {
      const int src = __ffsll(todo) - 1;
      todo &= todo - 1;
      const long long h0 = __shfl(r0, src), h1 = __shfl(r1, src);
      const int hs = __shfl(slot0, src);
      double v[KQ];
#pragma unroll
      for (int kk = 0; kk < KQ; ++kk) v[kk] = 0.0;
#pragma unroll 4
      for (long long r = h0 + sg; r <= h1; r += NSUB) {
#pragma unroll
        for (int kk = 0; kk < KQ; ++kk) {
          const int k = k0 + kk * oni::kWave;
          if (k < KS) v[kk] += scratch[(2 * r + (r == h0 ? hs : 0)) * KS + k];
        }
      }
#pragma unroll
      for (int kk = 0; kk < KQ; ++kk) {
#pragma unroll
        for (int m = G; m < oni::kWave; m <<= 1) v[kk] += __shfl_xor(v[kk], m);
        if (sg == src / G) acc[kk] = v[kk];
      }
    }
    if (write) {
#pragma unroll
      for (int kk = 0; kk < KQ; ++kk) {
        const int k = k0 + kk * oni::kWave;
        if (k < KS) ss[w * KS + k] = (float)((double)table[w * KS + k] * acc[kk]);
      }
    }
  }
}

// column partials of 256-word tiles: thread = (row group, column), groups added in group order
__global__ __launch_bounds__(kBlock) void k_vem_colpart(const float* __restrict__ ss, int64_t V, int KS,
                                                        double* __restrict__ part) {
  __shared__ double s_part[kBlock];
  const int t = threadIdx.x, ng = kBlock / KS > 0 ? kBlock / KS : 1;  // KS ≤ 256
  const int g = t / KS, k = t - g * KS;
  const int64_t nT = (V + kColTile - 1) / kColTile;
  for (int64_t tile = blockIdx.x; tile < nT; tile += gridDim.x) {  // block-uniform trip count
    const int64_t w0 = tile * kColTile, w1 = w0 + kColTile < V ? w0 + kColTile : V;
    double x = 0.0;
    if (g < ng)
      for (int64_t w = w0 + g; w < w1; w += ng) x += (double)ss[w * KS + k];
    s_part[t] = x;
    __syncthreads();
    if (t < KS) {
      double y = s_part[t];
      for (int j = 1; j < ng; ++j) y += s_part[j * KS + t];
      part[tile * KS + t] = y;
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(kBlock) void k_vem_coltot(const double* __restrict__ part, int64_t nT, int KS, int K,
                                                       double* __restrict__ ssk) {
  const int k = threadIdx.x;
  if (k >= KS) return;
  double x = 0.0;
  if (k < K)
    for (int64_t t = 0; t < nT; ++t) x += part[t * KS + k];
  ssk[k] = x;
}

__global__ __launch_bounds__(kBlock) void k_vem_rows(const float* __restrict__ ss, const double* __restrict__ ssk,
                                                     int64_t V, int KS, int K, double beta, double vbeta,
                                                     float* __restrict__ table) {
  const int64_t n = (V + 1) * KS;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
    const int64_t w = i / KS;
    const int k = (int)(i - w * KS);
    float v = 0.f;
    if (k < K) v = (float)(((w < V ? (double)ss[i] : 0.0) + beta) / (ssk[k] + vbeta));
    table[i] = v;
  }
}

bool bad_ks(int KS, int K) { return K < 1 || K > KS || KS % 4 != 0 || KS > 256; }

}  // namespace

// one lane-group shape per row width: G lanes a row up to 32 columns, then the whole wave with
// KQ = 1, 2 or 4 columns a lane
#define ONI_VEM_SHAPES(KS_, CALL)        \
  if (KS_ <= 4) { CALL(4, 1) }           \
  else if (KS_ <= 8) { CALL(8, 1) }      \
  else if (KS_ <= 16) { CALL(16, 1) }    \
  else if (KS_ <= 32) { CALL(32, 1) }    \
  else if (KS_ <= 64) { CALL(64, 1) }    \
  else if (KS_ <= 128) { CALL(64, 2) }   \
  else { CALL(64, 4) }

// gamma f32 [D][KS] (the E-step's), table f32 [rows][KS], doc-major pdoc / pword / pcnt int32 [P],
// wm_pos int32 [P] (a permutation of 0 .. P−1) or null: e_out f32 [D][KS], q_out f32 [P] at wm_pos
// (or in the pairs' own order).
ONI_API int oni_vem_resp(const float* gamma, const float* table, int64_t rows, int KS, int K, const int32_t* pdoc,
                         const int32_t* pword, const int32_t* pcnt, const int32_t* wm_pos, int64_t P, int64_t D,
                         float* e_out, float* q_out, hipStream_t s) {
  if (bad_ks(KS, K) || P < 0 || D < 0 || D > 0x7FFFFFFFll || rows < 1 || rows > 0x7FFFFFFFll) return (int)hipErrorInvalidValue;
  if (D > 0 && (gamma == nullptr || e_out == nullptr)) return (int)hipErrorInvalidValue;
  if (P > 0 && (table == nullptr || pdoc == nullptr || pword == nullptr || pcnt == nullptr || q_out == nullptr || D == 0))
    return (int)hipErrorInvalidValue;
  if (D > 0) {
#define ONI_E(G_, KQ_) \
  k_vem_e<G_, KQ_><<<oni::grid_for((D + 64 / G_ - 1) / (64 / G_), kWaves, 4096), kBlock, 0, s>>>(gamma, D, KS, K, e_out);
    ONI_VEM_SHAPES(KS, ONI_E)
#undef ONI_E
  }
  if (P > 0) {
    const unsigned g = oni::grid_for(P, kBlock, 4096);
    const int32_t Di = (int32_t)D, Ri = (int32_t)rows;
#define ONI_Q(k_) \
  if (KS == k_) k_vem_q<k_><<<g, kBlock, 0, s>>>(e_out, table, KS, pdoc, pword, pcnt, wm_pos, P, Di, Ri, q_out); else
    ONI_Q(20) ONI_Q(56) ONI_Q(100)
#undef ONI_Q
    k_vem_q<0><<<g, kBlock, 0, s>>>(e_out, table, KS, pdoc, pword, pcnt, wm_pos, P, Di, Ri, q_out);
  }
  return (int)hipGetLastError();
}

// e f32 [D][KS], word-major q f32 / wdoc / wword int32 [P] (wword non-decreasing), word_pair_ptr
// int64 [V + 1] (0 .. P), table f32 [V + 1][KS]: ss_out f32 [V][KS] = table · Σ q·e per word.
// scratch: 2·⌈P/256⌉·KS doubles, uninitialised. grid: blocks of both passes (0: sized from P and
// V); the result does not depend on it.
ONI_API int oni_vem_wsum(const float* e, const float* q, const int32_t* wdoc, const int32_t* wword,
                         const int64_t* word_pair_ptr, const float* table, int64_t P, int64_t D, int64_t V, int KS,
                         int K, float* ss_out, double* scratch, int grid, hipStream_t s) {
  if (bad_ks(KS, K) || P < 0 || D < 0 || D > 0x7FFFFFFFll || V < 0 || V > 0x7FFFFFFFll || grid < 0 || grid > 65535)
    return (int)hipErrorInvalidValue;
  if (V == 0) return P == 0 ? 0 : (int)hipErrorInvalidValue;
  if (word_pair_ptr == nullptr || table == nullptr || ss_out == nullptr) return (int)hipErrorInvalidValue;
  if (P > 0 && (e == nullptr || q == nullptr || wdoc == nullptr || wword == nullptr || scratch == nullptr || D == 0))
    return (int)hipErrorInvalidValue;
  const WsumArgs a{e, q, wdoc, wword, table, ss_out, scratch, P, (int32_t)D, (int32_t)V, KS};
  const int64_t nspan = (P + kSpan - 1) / kSpan;
#define ONI_W(G_, KQ_)                                                                                              \
  if (P > 0) k_vem_wsum<G_, KQ_><<<grid > 0 ? (unsigned)grid : oni::grid_for(nspan, kWaves, 16384), kBlock, 0, s>>>(a); \
  k_vem_wcomb<G_, KQ_><<<grid > 0 ? (unsigned)grid : oni::grid_for((V + 64 / G_ - 1) / (64 / G_), kWaves, 4096),    \
                         kBlock, 0, s>>>(word_pair_ptr, V, KS, table, scratch, ss_out);
  ONI_VEM_SHAPES(KS, ONI_W)
#undef ONI_W
  return (int)hipGetLastError();
}

// ss f32 [V][KS]: table_out f32 [V + 1][KS] = (ss + β)/(ss_k + Vβ), row V = β/(ss_k + Vβ), zero past
// K; ssk_out f64 [KS] the column totals (zero past K). part: ⌈V/256⌉·KS doubles, uninitialised.
ONI_API int oni_vem_table(const float* ss, int64_t V, int KS, int K, double beta, float* table_out, double* ssk_out,
                          double* part, int grid, hipStream_t s) {
  if (bad_ks(KS, K) || V < 1 || V > 0x7FFFFFFFll || !(beta > 0.0) || grid < 0 || grid > 65535 || ss == nullptr ||
      table_out == nullptr || ssk_out == nullptr || part == nullptr)
    return (int)hipErrorInvalidValue;
  const int64_t nT = (V + kColTile - 1) / kColTile;
  k_vem_colpart<<<grid > 0 ? (unsigned)grid : oni::grid_for(nT, 1, 2048), kBlock, 0, s>>>(ss, V, KS, part);
  k_vem_coltot<<<1, kBlock, 0, s>>>(part, nT, KS, K, ssk_out);
  k_vem_rows<<<grid > 0 ? (unsigned)grid : oni::grid_for((V + 1) * KS, kBlock, 2048), kBlock, 0, s>>>(
      ss, ssk_out, V, KS, K, beta, (double)V * beta, table_out);
  return (int)hipGetLastError();
}
