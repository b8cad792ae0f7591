// Variational fold-in (`lda inf`, mean field): θ of new documents against a FROZEN word table, over
// the doc-major list of distinct (document, word, count) pairs. Deterministic, no seed, no sampler.
//
// Per document d with pairs p = (w_p, c_p) in corpus order, table rows φ_w (row V: unseen words,
// columns ≥ K zero) and doc-side prior row a_d (α, or the per-IP row of k_prior_rows):
//
//     γ_k ← a_dk + N_d / K                                   N_d = Σ c_p
//     iters times:  e_k = exp(ψ(γ_k) − max_j ψ(γ_j))
//                   s_p = Σ_k φ_{w_p,k} · e_k
//                   r_k = Σ_p (c_p / s_p) · φ_{w_p,k}
//                   γ_k ← a_dk + e_k · r_k
//     θ_dk = γ_k / Σ_j γ_j   (k < K), 0 for K ≤ k < KS
//
// the batch (Jacobi) form of lda-c's E-step (oni355/ref/vfold_spec.py is the specification). The
// iteration count is fixed: no per-document exit, so no result depends on a threshold decision.
//
// ONE launch runs every iteration of every document. Work split:
//
//   * A wave owns 16 consecutive documents (a block 64). It reads their 17 pair offsets once and
//     walks them in ROUNDS: the longest run of its next documents whose pairs fit 64 lanes (a
//     typical IP has ~7 pairs: one or two rounds). Ownership follows from the document id alone,
//     so nothing is searched and a document without pairs needs no special case (r = 0, γ = a).
//   * A round stages its pairs' table rows in LDS once (row stride 4·(KS/4 | 1) floats: an odd
//     number of 16-byte granules, so the row-per-lane float4 reads of neighbouring lanes fall on
//     different banks) and then alternates two lane mappings per iteration, all in LDS:
//        lane = pair            s_p over the pair's row and its document's e, q_p = c_p / s_p
//        lane = (document, k)   r_k walking the document's pairs in order, γ_k, ψ(γ_k);
//                               then max_j ψ by four lanes per document and e_k in place
//     γ, ψ and e share one [16][KS] buffer per wave. Rows wider than 64 floats are not staged:
//     they stay in L2 and are read from there each iteration (LDS would leave one wave per SIMD).
//   * A document with more than 64 pairs is left to the whole block after the rounds, again for
//     all iterations: lanes stride over its pairs (pair lo + 256·t + 64·wave + lane), each wave
//     transposes its 64 pairs with lane broadcasts into K partial sums held by lane = k, the four
//     waves' partials meet in LDS and are added in wave order, γ / ψ / e live in LDS. One block
//     re-reads at most (V + 1)·KS·4 bytes per iteration, mostly from L2.
//
// Every sum has an order fixed by pair index and document id: no atomics, the same bits from run
// to run. The rounds and the block path use block barriers; every loop around a barrier has a
// block-uniform trip count (the round loop through __syncthreads_or) and there is no early return.
//
// No MFMA: Φe and Φᵀ(c/s) are matrix-vector products over each document's own rows; a 64-pair
// tile's useful entries are block-diagonal, one block per document, so a matrix instruction would
// multiply mostly padding. Vector loads and stores only, no inline assembly.
//
// Word ids must lie in [0, rows of the table) and doc_pair_ptr must be non-decreasing from 0: the
// corpus builder guarantees both (as for k_foldin's tok_word), nothing here re-checks them.
#include "oni_common.h"

namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / oni::kWave;
constexpr int kSlots = 16;          // documents a wave owns
constexpr int kTile = oni::kWave;   // pairs of a round; a longer document takes the block path

struct VfoldArgs {
  const int32_t* pair_word;
  const int32_t* pair_cnt;
  const int64_t* doc_pair_ptr;
  const float* table;
  const float* prior;  // [D][KS] or nullptr: α
  float* theta;
  float* gamma;        // [D][KS] or nullptr
  int64_t D;
  int32_t KS, K, iters;
  float alpha;
};

// ψ(x), x > 0: recurrence up to x ≥ 6, then the asymptotic series (next term < 1e-10 there).
// The recurrence takes two steps per division, 1/x + 1/(x + 1) = (2x + 1)/(x(x + 1)): most γ of a
// short document sit near α and need all of them. The shift is a bounded loop, so no input (NaN,
// ≤ 0) can spin.
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

template <int KSMAX, bool STAGE>
struct alignas(16) WaveLds {
  float buf[kSlots * KSMAX];                      // γ / ψ / e of the wave's documents, [slot][KS]
  float rows[STAGE ? kTile * (KSMAX + 4) : 4];    // the round's table rows, padded stride
  float q[kTile];                                 // c_p / s_p
  int32_t word[kTile];
  int32_t cnt[kTile];
  float red[kSlots];                              // max ψ / Σγ per document
  long long ptr[kSlots + 1];                      // pair offsets of the wave's documents
  int32_t big[kSlots];                            // slots left to the block path
  int32_t nbig;
};

template <int KSMAX>
struct alignas(16) BlockLds {
  float psi[KSMAX];            // ψ(γ) between iterations, γ after the last
  float e[KSMAX];
  float part[kWaves][KSMAX];   // the waves' partial r
  long long red[kWaves];
};

__device__ __forceinline__ float prior_at(const VfoldArgs& a, int64_t d, int k) {
  return a.prior != nullptr ? a.prior[d * a.KS + k] : a.alpha;
}

// s = Σ_k row_k · e_k over KS columns (the padding columns of both are zero), k ascending
__device__ __forceinline__ float dot_e(const float* row, const float* e, int KS) {
  float s = 0.f;
  for (int j = 0; j < KS; j += 4) {
    const float4 x = *reinterpret_cast<const float4*>(row + j);
    const float4 y = *reinterpret_cast<const float4*>(e + j);
    s = fmaf(x.x, y.x, s);
    s = fmaf(x.y, y.y, s);
    s = fmaf(x.z, y.z, s);
    s = fmaf(x.w, y.w, s);
  }
  return s;
}

// One document of more than 64 pairs, by the whole block. Called by every thread of the block
// with the same arguments (block barriers inside).
template <int KSMAX>
__device__ void big_doc(const VfoldArgs& a, int64_t d, int64_t lo, int64_t hi, BlockLds<KSMAX>& B) {
  constexpr int KQ = (KSMAX + oni::kWave - 1) / oni::kWave;
  const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
  const int KS = a.KS, K = a.K;
  long long n = 0;
  for (int64_t p = lo + t; p < hi; p += kBlock) n += a.pair_cnt[p];
#pragma unroll
  for (int m = 1; m < oni::kWave; m <<= 1) n += __shfl_xor(n, m);
  if (lane == 0) B.red[wave] = n;
  __syncthreads();
  const long long N = B.red[0] + B.red[1] + B.red[2] + B.red[3];
  const float ak = t < K ? prior_at(a, d, t) : 0.f;
  if (t < KS && t < KSMAX) {
    float v = 0.f;
    if (t < K) {
      const float g = ak + (float)N / (float)K;
      v = a.iters > 0 ? digamma_f32(g) : g;
    }
    B.psi[t] = v;
  }
  __syncthreads();
  for (int it = 0; it < a.iters; ++it) {
    const bool last = it + 1 == a.iters;
    // every wave takes the maximum itself: no barrier, no partials
    float m = -__builtin_inff();
#pragma unroll
    for (int kk = 0; kk < KQ; ++kk) {
      const int k = lane + kk * oni::kWave;
      if (k < K) m = fmaxf(m, B.psi[k]);
    }
#pragma unroll
    for (int x = 1; x < oni::kWave; x <<= 1) m = fmaxf(m, __shfl_xor(m, x));
    const float ek = t < K ? expf(B.psi[t] - m) : 0.f;
    if (t < KS && t < KSMAX) B.e[t] = ek;
    __syncthreads();
    float acc[KQ];
#pragma unroll
    for (int kk = 0; kk < KQ; ++kk) acc[kk] = 0.f;
    for (int64_t base = lo + (int64_t)wave * kTile; base < hi; base += kBlock) {
      const int64_t p = base + lane;
      int w = 0;
      float q = 0.f;
      if (p < hi) {
        w = a.pair_word[p];
        q = (float)a.pair_cnt[p] / dot_e(a.table + (int64_t)w * KS, B.e, KS);
      }
      const int nv = hi - base < kTile ? (int)(hi - base) : kTile;
      for (int j = 0; j < nv; ++j) {  // the wave's pairs in order, lane = k
        const float qj = __shfl(q, j);
        const float* row = a.table + (int64_t)__shfl(w, j) * KS;
#pragma unroll
        for (int kk = 0; kk < KQ; ++kk) {
          const int k = lane + kk * oni::kWave;
          if (k < K) acc[kk] = fmaf(qj, row[k], acc[kk]);
        }
      }
    }
#pragma unroll
    for (int kk = 0; kk < KQ; ++kk) {
      const int k = lane + kk * oni::kWave;
      if (k < KSMAX) B.part[wave][k] = acc[kk];
    }
    __syncthreads();
    if (t < K) {
      const float r = ((B.part[0][t] + B.part[1][t]) + B.part[2][t]) + B.part[3][t];
      const float g = fmaf(ek, r, ak);
      B.psi[t] = last ? g : digamma_f32(g);
    }
    __syncthreads();
  }
  float sum = 0.f;
#pragma unroll
  for (int kk = 0; kk < KQ; ++kk) {
    const int k = lane + kk * oni::kWave;
    if (k < K) sum += B.psi[k];
  }
#pragma unroll
  for (int x = 1; x < oni::kWave; x <<= 1) sum += __shfl_xor(sum, x);
  if (t < KS && t < KSMAX) {
    const float g = t < K ? B.psi[t] : 0.f;
    a.theta[d * KS + t] = t < K ? g / sum : 0.f;
    if (a.gamma != nullptr) a.gamma[d * KS + t] = g;
  }
  __syncthreads();  // psi / e / red are reused by the block's next document
}

template <int KSMAX, bool STAGE>
__global__ __launch_bounds__(kBlock) void k_vfold(const VfoldArgs a) {
  __shared__ __attribute__((aligned(16))) WaveLds<KSMAX, STAGE> s_w[kWaves];
  __shared__ __attribute__((aligned(16))) BlockLds<KSMAX> s_b;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  WaveLds<KSMAX, STAGE>& L = s_w[wave];
  const int KS = a.KS, K = a.K, KS4 = KS >> 2;
  const int stride = 4 * (KS4 | 1);
  const uint32_t ks_inv = 0xFFFFFFFFu / (uint32_t)KS + 1u;  // ⌊i / KS⌋ = umulhi(i, ks_inv) for i < 2^24 / KS
  const int64_t d0 = ((int64_t)blockIdx.x * kWaves + wave) * kSlots;
  const int nd = d0 < a.D ? (a.D - d0 < kSlots ? (int)(a.D - d0) : kSlots) : 0;
  if (nd > 0 && lane <= nd) L.ptr[lane] = a.doc_pair_ptr[d0 + lane];
  __syncthreads();

  int s0 = 0, nbig = 0;
  for (;;) {
    // the wave's next round (wave-uniform): skip what the block path takes, then the longest run
    // of documents whose pairs fit the tile
    while (s0 < nd && L.ptr[s0 + 1] - L.ptr[s0] > kTile) {
      if (lane == 0) L.big[nbig] = s0;
      ++nbig;
      ++s0;
    }
    int s1 = s0;
    while (s1 < nd && L.ptr[s1 + 1] - L.ptr[s0] <= kTile) ++s1;
    if (!__syncthreads_or(s1 > s0)) break;  // block-uniform: no wave has a round left
    const int ns = s1 - s0, items = ns * KS;
    const int64_t p0 = ns > 0 ? (int64_t)L.ptr[s0] : 0;
    const int np = ns > 0 ? (int)(L.ptr[s1] - p0) : 0;
    int word = 0, cnt = 0, myslot = s0;
    if (lane < np) {
      word = a.pair_word[p0 + lane];
      cnt = a.pair_cnt[p0 + lane];
      L.word[lane] = word;
      L.cnt[lane] = cnt;
      for (int s = s0 + 1; s < s1; ++s) myslot += L.ptr[s] <= p0 + lane ? 1 : 0;
    }
    __syncthreads();
    if constexpr (STAGE) {
      for (int i = lane; i < np * KS4; i += oni::kWave) {
        const int r = i / KS4, c = (i - r * KS4) * 4;
        *reinterpret_cast<float4*>(L.rows + r * stride + c) =
            *reinterpret_cast<const float4*>(a.table + (int64_t)L.word[r] * KS + c);
      }
    }
    // γ0 = a + N_d / K (and its ψ); the padding columns of the buffer stay zero
    for (int i = lane; i < items; i += oni::kWave) {
      const int sl = s0 + (int)__umulhi((uint32_t)i, ks_inv), k = i - (sl - s0) * KS;
      float v = 0.f;
      if (k < K) {
        const int lo = (int)(L.ptr[sl] - p0), hi = (int)(L.ptr[sl + 1] - p0);
        long long N = 0;
        for (int p = lo; p < hi; ++p) N += L.cnt[p];
        const float g = prior_at(a, d0 + sl, k) + (float)N / (float)K;
        v = a.iters > 0 ? digamma_f32(g) : g;
      }
      L.buf[sl * KS + k] = v;
    }
    __syncthreads();
    const int rsl = s0 + (lane >> 2), rq = lane & 3;  // four lanes per document for max ψ and Σγ
    for (int it = 0; it < a.iters; ++it) {
      const bool last = it + 1 == a.iters;
      float m = -__builtin_inff();
      if (rsl < s1)
        for (int k = rq; k < K; k += 4) m = fmaxf(m, L.buf[rsl * KS + k]);
      m = fmaxf(m, __shfl_xor(m, 1));
      m = fmaxf(m, __shfl_xor(m, 2));
      if (rsl < s1 && rq == 0) L.red[rsl] = m;
      __syncthreads();
      for (int i = lane; i < items; i += oni::kWave) {
        const int sl = s0 + (int)__umulhi((uint32_t)i, ks_inv), k = i - (sl - s0) * KS;
        if (k < K) L.buf[sl * KS + k] = expf(L.buf[sl * KS + k] - L.red[sl]);
      }
      __syncthreads();
      if (lane < np) {  // lane = pair
        const float* row = STAGE ? L.rows + lane * stride : a.table + (int64_t)word * KS;
        L.q[lane] = (float)cnt / dot_e(row, L.buf + myslot * KS, KS);
      }
      __syncthreads();
      for (int i = lane; i < items; i += oni::kWave) {  // lane = (document, k)
        const int sl = s0 + (int)__umulhi((uint32_t)i, ks_inv), k = i - (sl - s0) * KS;
        if (k < K) {
          const int lo = (int)(L.ptr[sl] - p0), hi = (int)(L.ptr[sl + 1] - p0);
          float r = 0.f;
          for (int p = lo; p < hi; ++p) {
            const float x = STAGE ? L.rows[p * stride + k] : a.table[(int64_t)L.word[p] * KS + k];
            r = fmaf(L.q[p], x, r);
          }
          const float g = fmaf(L.buf[sl * KS + k], r, prior_at(a, d0 + sl, k));
          L.buf[sl * KS + k] = last ? g : digamma_f32(g);
        }
      }
      __syncthreads();
    }
    float sum = 0.f;
    if (rsl < s1)
      for (int k = rq; k < K; k += 4) sum += L.buf[rsl * KS + k];
    sum += __shfl_xor(sum, 1);
    sum += __shfl_xor(sum, 2);
    if (rsl < s1 && rq == 0) L.red[rsl] = sum;
    __syncthreads();
    for (int i = lane; i < items; i += oni::kWave) {
      const int sl = s0 + (int)__umulhi((uint32_t)i, ks_inv), k = i - (sl - s0) * KS;
      const float g = L.buf[sl * KS + k];  // 0 in the padding columns
      const int64_t o = (d0 + sl) * KS + k;
      a.theta[o] = k < K ? g / L.red[sl] : 0.f;
      if (a.gamma != nullptr) a.gamma[o] = g;
    }
    __syncthreads();  // the next round reuses the wave's buffers
    s0 = s1;
  }

  if (lane == 0) L.nbig = nbig;
  __syncthreads();
  for (int w = 0; w < kWaves; ++w) {
    const int nb = s_w[w].nbig;  // block-uniform
    for (int i = 0; i < nb; ++i) {
      const int sl = s_w[w].big[i];
      big_doc<KSMAX>(a, ((int64_t)blockIdx.x * kWaves + w) * kSlots + sl, s_w[w].ptr[sl], s_w[w].ptr[sl + 1], s_b);
    }
  }
}

}  // namespace

// pair_word / pair_cnt int32 [P] doc-major, doc_pair_ptr int64 [D + 1] (0 .. P, non-decreasing),
// table f32 [rows][KS] with every pair_word < rows, prior f32 [D][KS] or null (the flat α),
// theta_out f32 [D][KS], gamma_out f32 [D][KS] or null. Row widths up to 256.
ONI_API int oni_vfold(const int32_t* pair_word, const int32_t* pair_cnt, const int64_t* doc_pair_ptr, int64_t D,
                      const float* table, int KS, int K, float alpha, const float* prior, int iters, float* theta_out,
                      float* gamma_out, hipStream_t s) {
  if (K < 1 || K > KS || KS % 4 != 0 || KS > 256 || iters < 0 || D < 0 || D > 0x7FFFFFFFll * 32) return (int)hipErrorInvalidValue;
  if (D == 0) return 0;
  if (doc_pair_ptr == nullptr || table == nullptr || theta_out == nullptr) return (int)hipErrorInvalidValue;
  if (prior == nullptr && !(alpha > 0.f)) return (int)hipErrorInvalidValue;
  const VfoldArgs a{pair_word, pair_cnt, doc_pair_ptr, table, prior, theta_out, gamma_out, D, KS, K, iters, alpha};
  const unsigned grid = (unsigned)((D + kWaves * kSlots - 1) / (kWaves * kSlots));
  if (KS <= 32) k_vfold<32, true><<<grid, kBlock, 0, s>>>(a);
  else if (KS <= 64) k_vfold<64, true><<<grid, kBlock, 0, s>>>(a);
  else if (KS <= 128) k_vfold<128, false><<<grid, kBlock, 0, s>>>(a);
  else k_vfold<256, false><<<grid, kBlock, 0, s>>>(a);
  return (int)hipGetLastError();
}
