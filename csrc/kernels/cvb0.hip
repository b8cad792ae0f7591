// Batch CVB0 (collapsed variational Bayes, zeroth order; Asuncion et al. 2009): the deterministic
// mean-field counterpart of the collapsed Gibbs sampler, over the corpus' doc-major distinct
// (document, word, count) pairs p = (d_p, w_p, c_p). oni355/ref/cvb0_spec.py is the specification.
//
//     init    t0[w,k] = 1/V + u(w,k)         r_pk = t0[w_p,k] / Σ_j t0[w_p,j]              k_cvb_init
//     step    u_k = (max(n_dk − r_pk, 0) + α) · (max(n_wk − r_pk, 0) + β) / (max(n_k − r_pk, 0) + Vβ)
//             r_pk ← u_k / Σ_j u_j           n_dk' = Σ_{p in d} c_p · r_pk                  k_cvb_update, k_cvb_docs
//     end     θ_dk = (n_dk + α) / (N_d + Kα), 1/K for a document without pairs             k_cvb_theta
//
// Every pair is updated from the OLD counts (Jacobi), and a pair reads no r row but its own, so r is
// updated in place. The word counts n_wk and n_k are not made here: they are the segmented sum over
// the word-major pair list that k_vem_wsum / k_vem_wcomb and the table pass of vem.hip already are.
//
// k_cvb_update<KS>  KS ≤ 64: lane = pair, pair i on lane i mod 64 of wave ⌊i/64⌋ whatever the grid.
//                 The lane streams its own r row, its document's n_dk row (neighbouring lanes share
//                 it: cache) and gathers its word's n_wk row, all as 16-byte loads. n_k sits in LDS
//                 as f32 (every lane reads the same k: a broadcast). KS = 20 and 56 are compiled
//                 with the row of u in registers; any other width runs the dynamic form, which
//                 makes the row twice (Σu, then u / Σu) from the rows the first pass left in cache.
//                 u is f32, its row sum f64 (ascending k), r = u / f32(Σu) with a true division.
//                 New n_dk: c·r in f64 (exact: both are f32), one segmented inclusive scan per
//                 column keyed by pair_doc (six __shfl_up steps; which lanes take is found once per
//                 wave and shared by the columns). A segment strictly inside the wave is a whole
//                 document: rounded once and written to n_dk'[d] (the compiled widths collect the
//                 row and write 16 bytes at a time). A segment touching lane 0 is the wave's HEAD,
//                 one touching only lane 63 its TAIL: KS doubles in slot 2w or 2w + 1 of a scratch
//                 buffer nobody initialises. As in fit.hip and vem_bound.hip the slot of a
//                 document's part in a wave follows from the document's pair range alone.
// k_cvb_update_wide<KQ>  KS > 64: the wave owns 64 consecutive pairs and walks them one after the
//                 other, lane = column (KQ = ⌈KS/64⌉ columns a lane): pair ids come by lane
//                 broadcast, the three rows as coalesced 4-byte loads, Σu by an xor butterfly in f64
//                 (commutative adds: the same bits in every lane). Each lane carries its columns'
//                 f64 sums of the open document and flushes them where the document changes: whole,
//                 head or tail exactly as above. One lane a pair would hold 3 × 100 floats here:
//                 the resource table in docs/cvb0.md has the crossover.
// k_cvb_docs<G,KQ>  a wave takes 64 documents, finds those the update pass did not finish (pairs in
//                 more than one wave, or touching a wave's edge; documents without pairs get
//                 zeros) and adds each one's records in wave order: groups of G = next-pow2(KS)
//                 lanes stride over the records, lane = column, then a fixed xor butterfly over the
//                 groups. A 10^5-pair document is 1600 records read 64/G at a time, not a chain of
//                 10^5 adds. One rounding to f32.
// k_cvb_init      lane = pair: Σ_j t0 and t0 / Σ in f64 from the hash (oni::mix32, oni::u01), so the
//                 row carries one rounding. A pair naming a word outside [0, V) gets a zero row.
// k_cvb_theta     thread = element of θ, f64 arithmetic rounded once.
//
// Which values are added, and in what order, follows from pair index and document id only: no
// atomics, the same bits whatever the grid and from run to run. Barriers: one __syncthreads in each
// update kernel, after n_k is staged and BEFORE its loop; every thread of the block reaches it,
// nothing returns before it, and no loop surrounds it. The loops themselves hold wave shuffles
// only: k_cvb_update's trip count is kept block-uniform and a wave past the end skips the body as a
// whole; k_cvb_update_wide and k_cvb_docs stride whole waves over tiles, so their trip counts, the
// pair walk (bounded by the tile's pair count) and the work list (a ballot) are wave-uniform.
//
// No MFMA: per pair the work is an elementwise product of three gathered rows and a normalisation;
// there is no shared operand to form a matrix product with. Vector loads and stores only, no inline
// assembly.
//
// Pairs naming a document outside [0, D) or a word outside [0, V) contribute nothing and nothing is
// read or written through them (their r rows stay as they are).
#include "oni_common.h"

namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / oni::kWave;
constexpr int kMaxKS = 256;

struct CvbArgs {
  float* r;                 // [P][KS], updated in place
  const float* ndk;         // [D][KS]
  const float* nwk;         // [V][KS]
  const double* nk;         // [KS]
  const int32_t* pdoc;      // [P] non-decreasing
  const int32_t* pword;     // [P]
  const int32_t* pcnt;      // [P]
  float* ndk_new;           // [D][KS]
  double* wrec;             // [2·⌈P/64⌉][KS]
  int64_t P;
  int32_t D, V, KS, K;
  float alpha, beta, vbeta;
};

// one column of the CVB0 conditional from the old counts, the pair's own share taken out
__device__ __forceinline__ float cvb_u(float r, float nd, float nw, float nk, const CvbArgs& a) {
  const float x = fmaxf(nd - r, 0.f) + a.alpha;
  const float y = fmaxf(nw - r, 0.f) + a.beta;
  const float z = fmaxf(nk - r, 0.f) + a.vbeta;
  return (x * y) / z;
}

__device__ __forceinline__ float comp4(const float4& v, int t) { return t == 0 ? v.x : (t == 1 ? v.y : (t == 2 ? v.z : v.w)); }

template <int KS>
__global__ __launch_bounds__(kBlock) void k_cvb_update(const CvbArgs a) {
  constexpr bool kRegs = KS > 0;
  constexpr int NR = kRegs ? KS : 4;
  __shared__ float s_nk[kMaxKS];
  const int ks = kRegs ? KS : a.KS;
  const int K = a.K;
  for (int k = threadIdx.x; k < ks; k += kBlock) s_nk[k] = (float)a.nk[k];
  __syncthreads();
  const int lane = threadIdx.x & (oni::kWave - 1);
  for (int64_t base = (int64_t)blockIdx.x * kBlock; base < a.P; base += (int64_t)gridDim.x * kBlock) {
    const int64_t i = base + threadIdx.x;
    if (i - lane >= a.P) continue;  // a wave past the end (wave-uniform)
    int doc = -1;
    bool live = false;
    double c = 0.0;
    const float *dp = nullptr, *wp = nullptr;
    float* rp = nullptr;
    if (i < a.P) {
      const int32_t d = a.pdoc[i], w = a.pword[i];
      if ((uint32_t)d < (uint32_t)a.D) {
        doc = d;
        if ((uint32_t)w < (uint32_t)a.V) {
          live = true;
          c = (double)a.pcnt[i];
          rp = a.r + i * ks;
          dp = a.ndk + (int64_t)d * ks;
          wp = a.nwk + (int64_t)w * ks;
        }
      }
    }
    float u[NR] = {};  // the row of u, then of r, then of the document sums (compiled widths)
    double S = 0.0;
    if (live) {
#pragma unroll
      for (int j = 0; j < ks; j += 4) {
        const float4 rr = *reinterpret_cast<const float4*>(rp + j);
        const float4 nd = *reinterpret_cast<const float4*>(dp + j);
        const float4 nw = *reinterpret_cast<const float4*>(wp + j);
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          const float v = j + t < K ? cvb_u(comp4(rr, t), comp4(nd, t), comp4(nw, t), s_nk[j + t], a) : 0.f;
          S += (double)v;
          if constexpr (kRegs) u[j + t] = v;
        }
      }
    }
    const float Sf = (float)S;
    if (live) {
#pragma unroll
      for (int j = 0; j < ks; j += 4) {
        float4 o;
        if constexpr (kRegs) {
          o = make_float4(u[j] / Sf, u[j + 1] / Sf, u[j + 2] / Sf, u[j + 3] / Sf);
          u[j] = o.x, u[j + 1] = o.y, u[j + 2] = o.z, u[j + 3] = o.w;
        } else {  // the row again, from the old r of these four columns, before they are overwritten
          const float4 rr = *reinterpret_cast<const float4*>(rp + j);
          const float4 nd = *reinterpret_cast<const float4*>(dp + j);
          const float4 nw = *reinterpret_cast<const float4*>(wp + j);
          float v[4];
#pragma unroll
          for (int t = 0; t < 4; ++t)
            v[t] = j + t < K ? cvb_u(comp4(rr, t), comp4(nd, t), comp4(nw, t), s_nk[j + t], a) / Sf : 0.f;
          o = make_float4(v[0], v[1], v[2], v[3]);
        }
        *reinterpret_cast<float4*>(rp + j) = o;
      }
    }
    // the segmented scan's shape, once for all columns: pair_doc is non-decreasing, so equal keys
    // s lanes apart mean one segment in between
    bool take[6];
#pragma unroll
    for (int s = 0; s < 6; ++s) {
      const int od = __shfl_up(doc, 1 << s);  // by every lane, before the test: a shuffle reads no inactive lane
      take[s] = lane >= (1 << s) && od == doc;
    }
    const int prev = __shfl_up(doc, 1), next = __shfl_down(doc, 1);
    const bool first = lane == 0 || prev != doc;
    const bool last = (lane == oni::kWave - 1 || next != doc) && doc >= 0;
    const uint64_t firsts = __ballot(first);
    const int fl = 63 - __clzll((long long)(firsts & (~0ull >> (63 - lane))));  // the segment's first lane
    const bool whole = last && fl != 0 && lane != oni::kWave - 1;
    const bool rec = last && !whole;
    double* rec_p = a.wrec + (2 * (i >> 6) + (fl != 0 ? 1 : 0)) * ks;
    float* out_p = a.ndk_new + (int64_t)(doc < 0 ? 0 : doc) * ks;
#pragma unroll
    for (int j = 0; j < ks; j += 4) {
      float4 rr = make_float4(0.f, 0.f, 0.f, 0.f);
      if (!kRegs && live) rr = *reinterpret_cast<const float4*>(rp + j);  // the lane's own store, back from cache
      float o[4];
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        float rn;
        if constexpr (kRegs) rn = u[j + t];
        else rn = comp4(rr, t);
        double v = live ? c * (double)rn : 0.0;
#pragma unroll
        for (int s = 0; s < 6; ++s) {
          const double up = __shfl_up(v, 1 << s);
          if (take[s]) v = up + v;
        }
        if (rec) rec_p[j + t] = v;
        o[t] = (float)v;
      }
      if (whole) *reinterpret_cast<float4*>(out_p + j) = make_float4(o[0], o[1], o[2], o[3]);
    }
  }
}

template <int KQ>
__device__ __forceinline__ void wide_flush(const CvbArgs& a, int d, int64_t tile, bool head, bool tail, int lane,
                                           const double (&acc)[KQ]) {
  if (d < 0) return;
#pragma unroll
  for (int kk = 0; kk < KQ; ++kk) {
    const int k = lane + kk * oni::kWave;
    if (k < a.KS) {
      if (head || tail) a.wrec[(2 * tile + (head ? 0 : 1)) * a.KS + k] = acc[kk];
      else a.ndk_new[(int64_t)d * a.KS + k] = (float)acc[kk];
    }
  }
}

template <int KQ>
__global__ __launch_bounds__(kBlock) void k_cvb_update_wide(const CvbArgs a) {
  __shared__ float s_nk[kMaxKS];
  const int ks = a.KS, K = a.K;
  for (int k = threadIdx.x; k < ks; k += kBlock) s_nk[k] = (float)a.nk[k];
  __syncthreads();
  const int lane = threadIdx.x & (oni::kWave - 1), wave = threadIdx.x / oni::kWave;
  float nk[KQ];
#pragma unroll
  for (int kk = 0; kk < KQ; ++kk) nk[kk] = lane + kk * oni::kWave < ks ? s_nk[lane + kk * oni::kWave] : 0.f;
  const int64_t nW = (a.P + oni::kWave - 1) / oni::kWave;
  for (int64_t tile = (int64_t)blockIdx.x * kWaves + wave; tile < nW; tile += (int64_t)gridDim.x * kWaves) {
    const int64_t base = tile * oni::kWave;
    const int nv = a.P - base < oni::kWave ? (int)(a.P - base) : oni::kWave;
    int dv = -1, wv = -1, cv = 0;
    if (lane < nv) {
      const int32_t d = a.pdoc[base + lane], w = a.pword[base + lane];
      if ((uint32_t)d < (uint32_t)a.D) {
        dv = d;
        if ((uint32_t)w < (uint32_t)a.V) wv = w;
      }
      cv = a.pcnt[base + lane];
    }
    double acc[KQ];
#pragma unroll
    for (int kk = 0; kk < KQ; ++kk) acc[kk] = 0.0;
    int cur = __shfl(dv, 0);
    bool head = true;  // the open segment touches the tile's first pair
    for (int j = 0; j < nv; ++j) {
      const int d = __shfl(dv, j), w = __shfl(wv, j);
      const double c = (double)__shfl(cv, j);
      if (d != cur) {
        wide_flush<KQ>(a, cur, tile, head, false, lane, acc);
#pragma unroll
        for (int kk = 0; kk < KQ; ++kk) acc[kk] = 0.0;
        cur = d;
        head = false;
      }
      if (d < 0 || w < 0) continue;  // wave-uniform
      float* rp = a.r + (base + j) * ks;
      const float* dp = a.ndk + (int64_t)d * ks;
      const float* wp = a.nwk + (int64_t)w * ks;
      float u[KQ];
      double S = 0.0;
#pragma unroll
      for (int kk = 0; kk < KQ; ++kk) {
        const int k = lane + kk * oni::kWave;
        u[kk] = k < K ? cvb_u(rp[k], dp[k], wp[k], nk[kk], a) : 0.f;
        S += (double)u[kk];
      }
#pragma unroll
      for (int m = 1; m < oni::kWave; m <<= 1) S += __shfl_xor(S, m);
      const float Sf = (float)S;
#pragma unroll
      for (int kk = 0; kk < KQ; ++kk) {
        const int k = lane + kk * oni::kWave;
        const float rn = u[kk] / Sf;
        if (k < ks) rp[k] = rn;
        acc[kk] += c * (double)rn;
      }
    }
    wide_flush<KQ>(a, cur, tile, head, !head && nv == oni::kWave, lane, acc);
  }
}

template <int G, int KQ>
__global__ __launch_bounds__(kBlock) void k_cvb_docs(const int64_t* __restrict__ dptr, int64_t P, int64_t D, int KS,
                                                     const double* __restrict__ wrec, float* __restrict__ ndk_new) {
  constexpr int NSUB = oni::kWave / G;
  const int lane = threadIdx.x & (oni::kWave - 1), wave = threadIdx.x / oni::kWave;
  const int sg = lane / G, k0 = lane % G;
  for (int64_t base = ((int64_t)blockIdx.x * kWaves + wave) * oni::kWave; base < D;
       base += (int64_t)gridDim.x * kWaves * oni::kWave) {
    const int64_t d = base + lane;
    long long w0 = 0, w1 = -1;  // no records: zeros
    int slot0 = 0;              // the slot of the document's part in its first wave (head in every later wave)
    bool need = false;
    if (d < D) {
      int64_t lo = dptr[d], hi = dptr[d + 1];
      lo = lo < 0 ? 0 : (lo > P ? P : lo);
      hi = hi < lo ? lo : (hi > P ? P : hi);
      need = true;
      if (lo < hi) {
        w0 = lo >> 6;
        w1 = (hi - 1) >> 6;
        slot0 = (lo & 63) != 0 ? 1 : 0;
        if (w0 == w1 && slot0 == 1 && ((hi - 1) & 63) != 63) need = false;  // k_cvb_update wrote the row
      }
    }
    uint64_t todo = __ballot(need);
    while (todo) {
      const int src = __ffsll((unsigned long long)todo) - 1;
      todo &= todo - 1;
      const long long h0 = __shfl(w0, src), h1 = __shfl(w1, src);
      const int hs = __shfl(slot0, src);
      double v[KQ];
#pragma unroll
      for (int kk = 0; kk < KQ; ++kk) v[kk] = 0.0;
#pragma unroll 4
      for (long long w = h0 + sg; w <= h1; w += NSUB) {
#pragma unroll
        for (int kk = 0; kk < KQ; ++kk) {
          const int k = k0 + kk * oni::kWave;
          if (k < KS) v[kk] += wrec[(2 * w + (w == h0 ? hs : 0)) * KS + k];
        }
      }
#pragma unroll
      for (int kk = 0; kk < KQ; ++kk) {
#pragma unroll
        for (int m = G; m < oni::kWave; m <<= 1) v[kk] += __shfl_xor(v[kk], m);
        const int k = k0 + kk * oni::kWave;
        if (sg == 0 && k < KS) ndk_new[(base + src) * KS + k] = (float)v[kk];
      }
    }
  }
}

__global__ __launch_bounds__(kBlock) void k_cvb_init(const int32_t* __restrict__ pword, int64_t P, int32_t V, int KS,
                                                     int K, float* __restrict__ r) {
  const double invV = 1.0 / (double)V;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < P; i += (int64_t)gridDim.x * kBlock) {
    const int32_t w = pword[i];
    const bool ok = (uint32_t)w < (uint32_t)V;
    const uint32_t h0 = (uint32_t)w * (uint32_t)K;
    double S = 0.0;
    if (ok)
      for (int k = 0; k < K; ++k) S += invV + (double)oni::u01(oni::mix32(h0 + (uint32_t)k));
    for (int j = 0; j < KS; j += 4) {
      float v[4];
#pragma unroll
      for (int t = 0; t < 4; ++t)
        v[t] = ok && j + t < K ? (float)((invV + (double)oni::u01(oni::mix32(h0 + (uint32_t)(j + t)))) / S) : 0.f;
      *reinterpret_cast<float4*>(r + i * KS + j) = make_float4(v[0], v[1], v[2], v[3]);
    }
  }
}

__global__ __launch_bounds__(kBlock) void k_cvb_theta(const float* __restrict__ ndk, const int64_t* __restrict__ doc_len,
                                                      int64_t D, int KS, int K, double alpha,
                                                      float* __restrict__ theta) {
  const int64_t n = D * KS;
  for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < n; e += (int64_t)gridDim.x * kBlock) {
    const int64_t d = e / KS;
    const int k = (int)(e - d * KS);
    const int64_t N = doc_len[d];
    float v = 0.f;
    if (k < K) v = N > 0 ? (float)(((double)ndk[e] + alpha) / ((double)N + (double)K * alpha)) : (float)(1.0 / (double)K);
    theta[e] = v;
  }
}

}  // namespace

// the lane-group ladder of vem.hip (kept as a copy so that file stays as it is)
#define ONI_CVB_SHAPES(KS_, CALL)        \
  if (KS_ <= 4) { CALL(4, 1) }           \
  else if (KS_ <= 8) { CALL(8, 1) }      \
  else if (KS_ <= 16) { CALL(16, 1) }    \
  else if (KS_ <= 32) { CALL(32, 1) }    \
  else if (KS_ <= 64) { CALL(64, 1) }    \
  else if (KS_ <= 128) { CALL(64, 2) }   \
  else { CALL(64, 4) }

// r f32 [P][KS] from the hash init of the doc-major pairs' words.
ONI_API int oni_cvb0_init(const int32_t* pword, int64_t P, int64_t V, int KS, int K, float* r, hipStream_t s) {
  if (K < 1 || K > KS || KS % 4 != 0 || KS > kMaxKS || P < 0 || V < 1 || V > 0x7FFFFFFFll ||
      (uint64_t)V * (uint64_t)K > 0xFFFFFFFFull)
    return (int)hipErrorInvalidValue;
  if (P == 0) return 0;
  if (pword == nullptr || r == nullptr) return (int)hipErrorInvalidValue;
  k_cvb_init<<<oni::grid_for(P, kBlock, 4096), kBlock, 0, s>>>(pword, P, (int32_t)V, KS, K, r);
  return (int)hipGetLastError();
}

// One Jacobi step: r f32 [P][KS] in place from ndk f32 [D][KS], nwk f32 [V][KS], nk f64 [KS] and the
// doc-major pairs (pdoc non-decreasing, doc_pair_ptr int64 [D + 1] their ranges); ndk_new f32 [D][KS]
// = Σ_{p in d} c_p · r_pk of the new r. scratch: 2·⌈P/64⌉·KS doubles (scratch_len says how many
// there are), uninitialised. grid: blocks of both passes (0: sized from P and D); the result does
// not depend on it.
ONI_API int oni_cvb0_update(float* r, const float* ndk, const float* nwk, const double* nk, const int32_t* pdoc,
                            const int32_t* pword, const int32_t* pcnt, const int64_t* doc_pair_ptr, int64_t P,
                            int64_t D, int64_t V, int KS, int K, double alpha, double beta, float* ndk_new,
                            double* scratch, int64_t scratch_len, int grid, hipStream_t s) {
  if (K < 1 || K > KS || KS % 4 != 0 || KS > kMaxKS || P < 0 || D < 0 || D > 0x7FFFFFFFll || V < 1 ||
      V > 0x7FFFFFFFll || !(alpha > 0.0) || !(beta > 0.0) || grid < 0 || grid > 65535 || nk == nullptr)
    return (int)hipErrorInvalidValue;
  if (D > 0 && (ndk == nullptr || ndk_new == nullptr || doc_pair_ptr == nullptr)) return (int)hipErrorInvalidValue;
  if (P > 0 && (r == nullptr || nwk == nullptr || pdoc == nullptr || pword == nullptr || pcnt == nullptr || D == 0 ||
                scratch == nullptr))
    return (int)hipErrorInvalidValue;
  const int64_t nW = (P + oni::kWave - 1) / oni::kWave;
  if (scratch_len < 2 * nW * KS) return (int)hipErrorInvalidValue;
  if (P > 0) {
    CvbArgs a;
    a.r = r, a.ndk = ndk, a.nwk = nwk, a.nk = nk, a.pdoc = pdoc, a.pword = pword, a.pcnt = pcnt;
    a.ndk_new = ndk_new, a.wrec = scratch, a.P = P, a.D = (int32_t)D, a.V = (int32_t)V, a.KS = KS, a.K = K;
    a.alpha = (float)alpha, a.beta = (float)beta, a.vbeta = (float)((double)V * beta);
    if (KS <= 64) {
      const unsigned g = grid > 0 ? (unsigned)grid : oni::grid_for(P, kBlock, 16384);
      if (KS == 20) k_cvb_update<20><<<g, kBlock, 0, s>>>(a);
      else if (KS == 56) k_cvb_update<56><<<g, kBlock, 0, s>>>(a);
      else k_cvb_update<0><<<g, kBlock, 0, s>>>(a);
    } else {
      const unsigned g = grid > 0 ? (unsigned)grid : oni::grid_for(nW, kWaves, 16384);
      if (KS <= 128) k_cvb_update_wide<2><<<g, kBlock, 0, s>>>(a);
      else k_cvb_update_wide<4><<<g, kBlock, 0, s>>>(a);
    }
  }
  if (D > 0) {
    const unsigned g = grid > 0 ? (unsigned)grid : oni::grid_for((D + 63) / 64, kWaves, 4096);
#define ONI_D(G_, KQ_) k_cvb_docs<G_, KQ_><<<g, kBlock, 0, s>>>(doc_pair_ptr, P, D, KS, scratch, ndk_new);
    ONI_CVB_SHAPES(KS, ONI_D)
#undef ONI_D
  }
  return (int)hipGetLastError();
}

// theta f32 [D][KS] = (ndk + α) / (doc_len + Kα), 1/K where doc_len is 0, zero past K.
ONI_API int oni_cvb0_theta(const float* ndk, const int64_t* doc_len, int64_t D, int KS, int K, double alpha,
                           float* theta, hipStream_t s) {
  if (K < 1 || K > KS || KS % 4 != 0 || KS > kMaxKS || D < 0 || !(alpha > 0.0)) return (int)hipErrorInvalidValue;
  if (D == 0) return 0;
  if (ndk == nullptr || doc_len == nullptr || theta == nullptr) return (int)hipErrorInvalidValue;
  k_cvb_theta<<<oni::grid_for(D * KS, kBlock, 4096), kBlock, 0, s>>>(ndk, doc_len, D, KS, K, alpha, theta);
  return (int)hipGetLastError();
}
