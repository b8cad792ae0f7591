// Variational fold-in with a warm start and a per-document exit: k_vfold's E-step (vfold.hip), started
// from a given γ and stopped per document (oni355/ref/vfold_exit_spec.py is the specification).
//
// Per document d, with update() exactly one iteration of k_vfold (e = exp(ψ(γ) − max ψ), s_p = φ_p·e,
// r_k = Σ_p (c_p / s_p) φ_pk over the pairs in corpus order, γ_k ← a_dk + e_k r_k):
//
//     γ ← gamma0[d]  if given, else  a_d + N_d / K
//     up to max_iters times, while d is active:
//         γ_new = update(γ);  change = Σ_k |γ_new,k − γ_k|;  total = Σ_k γ_new,k;  γ ← γ_new
//         d freezes when change ≤ tol · total
//     θ_dk = γ_k / Σ_j γ_j,  n_it[d] = updates received
//
// This is the γ-change rule, relative to Σγ; it is not lda-c's relative change of the per-document
// likelihood (a lgamma row per iteration). With tol = 0 a document freezes only on an exact fixed
// point, so θ and γ are bit for bit k_vfold's with iters = max_iters.
//
// Kept from k_vfold, operation for operation, because the bitwise promises rest on it: digamma_f32
// (a copy, as vem.hip keeps one), dot_e's k-ascending fma chain, r_k over the document's pairs in
// corpus order, the block path's pair striding and its wave-ordered join of four partials, the
// padded LDS row staging for KS ≤ 64 (unstaged above), the 16 documents a wave owns by document id
// and rounds of ≤ 64 pairs.
//
// What differs is that documents of one round stop at different iterations, so the waves of a
// block leave their iteration loops at different times. The design chosen: KEEP the 256-thread
// block and the single launch, and put NO block barrier inside a round. Everything a round touches
// in LDS is wave-private (WaveLds below), and a wave's passes are ordered by wave_sync(): a
// wavefront-scope release/acquire fence pair around __builtin_amdgcn_wave_barrier(). The LDS
// serves one wave's accesses in issue order, so the fence only has to stop the compiler from
// moving accesses across it. The alternative (one wave per block plus a second launch for the
// documents over 64 pairs, with a list of them built per corpus) was not taken: it needs a
// host-side list and a size read per corpus, changes the op's signature into a two-step one, and
// gives up the sharing of one block's LDS allocation among four waves for nothing the fences do
// not already give.
//
// Per-document state of a round: L.gam [16][KS] holds γ itself across iterations (L.buf is reused
// for ψ, e and |Δ|, as k_vfold reuses it for ψ and e), L.act[slot] is the active flag. One
// iteration is six wave-ordered passes; the lanes of a frozen document skip all of them and its
// staged rows go unused:
//     lane = (document, k)   buf ← ψ(gam)
//     four lanes / document  max ψ → red
//     lane = (document, k)   buf ← exp(buf − red)
//     lane = pair            q_p = c_p / dot_e(row_p, e)
//     lane = (document, k)   r_k, γ_new; buf ← |γ_new − gam|, gam ← γ_new
//     four lanes / document  Σ buf and Σ gam over k = rq, rq + 4, … then the two xor steps; quad
//                            lane 0 counts the update and, on change ≤ tol · total, clears act
// and the loop ends when __ballot over the quad leaders finds no active slot, or at max_iters.
//
// Block path (a document over 64 pairs, after the rounds, the whole block, one at a time): thread
// t < K carries γ_t in a register. The waves' partial Σ|Δ| and Σγ meet in LDS like part[][] and
// are added in wave order by thread 0, which writes the exit decision into ONE LDS word; every
// thread reads that word after a barrier and takes the same branch. No thread recomputes it.
//
// Barriers and why each loop around one is uniform over the barrier's scope:
//   * k_vfold_exit has two __syncthreads outside every loop: after the pair offsets are read, and
//     between "this wave has no round left" and the block path. Every wave executes both once; the
//     round loop between them contains no block barrier and no early return.
//   * wave_sync() inside the round loop and the iteration loop: scope is the wave. s0, s1, np, it,
//     max_iters and the __ballot result are wave-uniform values, so all 64 lanes take every loop
//     exit together.
//   * the block path's loops over (wave w, its big documents i): the counts s_w[w].nbig are read
//     from LDS after the second barrier, the same for all 256 threads.
//   * big_doc's iteration loop: the trip count is max_iters (a kernel argument) cut short by
//     B.stop, an LDS word written by thread 0 alone between two barriers and read by all threads
//     after the second; it is next written after the following iteration's first barrier, when
//     every thread has read it. The pair loops inside have no barrier.
//
// Every sum has an order fixed by pair index, k and wave id: no atomics, the same bits from run to
// run, and a document's (γ, θ, n_it) depend on its own inputs alone, not on D, the grid or the
// documents that share its wave (a frozen neighbour changes which lanes idle, not what the others
// compute).
//
// No MFMA: Φe and Φᵀ(c/s) are matrix-vector products over each document's own rows; a 64-pair
// tile's useful entries are block-diagonal, one block per document, so a matrix instruction would
// multiply mostly padding. Vector loads and stores only, no inline assembly.
//
// Word ids must lie in [0, rows of the table) and doc_pair_ptr must be non-decreasing from 0, as
// for k_vfold; gamma0, where given, must be > 0 in its first K columns (its padding is ignored).
#include "oni_common.h"

namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / oni::kWave;
constexpr int kSlots = 16;          // documents a wave owns
constexpr int kTile = oni::kWave;   // pairs of a round; a longer document takes the block path

struct VfoldExitArgs {
  const int32_t* pair_word;
  const int32_t* pair_cnt;
  const int64_t* doc_pair_ptr;
  const float* table;
  const float* prior;   // [D][KS] or nullptr: α
  const float* gamma0;  // [D][KS] or nullptr: the cold start a + N/K
  float* theta;
  float* gamma;
  int32_t* n_it;
  int64_t D;
  int32_t KS, K, max_iters;
  float alpha, tol;
};

// ψ(x), x > 0: k_vfold's series, operation for operation (see vfold.hip)
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

// orders one wave's LDS traffic: what its lanes wrote before is what its lanes read after
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

template <int KSMAX, bool STAGE>
struct alignas(16) WaveLds {
  float buf[kSlots * KSMAX];                      // ψ / e / |Δ| of the wave's documents, [slot][KS]
  float gam[kSlots * KSMAX];                      // γ, [slot][KS], zero in the padding columns
  float rows[STAGE ? kTile * (KSMAX + 4) : 4];    // the round's table rows, padded stride
  float q[kTile];                                 // c_p / s_p
  int32_t word[kTile];
  int32_t cnt[kTile];
  float red[kSlots];                              // max ψ / Σγ per document
  int32_t act[kSlots];                            // 1 while the document still iterates
  long long ptr[kSlots + 1];                      // pair offsets of the wave's documents
  int32_t big[kSlots];                            // slots left to the block path
  int32_t nbig;
};

template <int KSMAX>
struct alignas(16) BlockLds {
  float psi[KSMAX];
  float e[KSMAX];
  float gam[KSMAX];            // γ, zero in the padding columns
  float part[kWaves][KSMAX];   // the waves' partial r
  float chg[kWaves], tot[kWaves];
  long long red[kWaves];
  int32_t stop;                // the exit decision of the iteration, written by thread 0
};

__device__ __forceinline__ float prior_at(const VfoldExitArgs& a, int64_t d, int k) {
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

// a γ0 row's four columns from c on, the padding columns forced to zero
__device__ __forceinline__ float4 gamma0_at(const VfoldExitArgs& a, int64_t d, int c) {
  float4 v = *reinterpret_cast<const float4*>(a.gamma0 + d * a.KS + c);
  if (c + 0 >= a.K) v.x = 0.f;
  if (c + 1 >= a.K) v.y = 0.f;
  if (c + 2 >= a.K) v.z = 0.f;
  if (c + 3 >= a.K) v.w = 0.f;
  return v;
}

// One document of more than 64 pairs, by the whole block. Called by every thread of the block
// with the same arguments (block barriers inside).
template <int KSMAX>
__device__ void big_doc(const VfoldExitArgs& a, int64_t d, int64_t lo, int64_t hi, BlockLds<KSMAX>& B) {
  constexpr int KQ = (KSMAX + oni::kWave - 1) / oni::kWave;
  const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
  const int KS = a.KS, K = a.K;
  const float ak = t < K ? prior_at(a, d, t) : 0.f;
  if (a.gamma0 != nullptr) {
    if (t < (KS >> 2)) *reinterpret_cast<float4*>(B.gam + 4 * t) = gamma0_at(a, d, 4 * t);
  } else {
    long long n = 0;
    for (int64_t p = lo + t; p < hi; p += kBlock) n += a.pair_cnt[p];
#pragma unroll
    for (int m = 1; m < oni::kWave; m <<= 1) n += __shfl_xor(n, m);
    if (lane == 0) B.red[wave] = n;
    __syncthreads();
    const long long N = B.red[0] + B.red[1] + B.red[2] + B.red[3];
    if (t < KS && t < KSMAX) B.gam[t] = t < K ? ak + (float)N / (float)K : 0.f;
  }
  __syncthreads();
  float g = t < K ? B.gam[t] : 0.f;  // thread t carries γ_t
  if (t < KS && t < KSMAX) B.psi[t] = t < K && a.max_iters > 0 ? digamma_f32(g) : 0.f;
  __syncthreads();
  int nit = 0;
  for (int it = 0; it < a.max_iters; ++it) {
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
    float dk = 0.f, gk = 0.f;  // this thread's |Δ| and γ_new, 0 past K
    if (t < K) {
      const float r = ((B.part[0][t] + B.part[1][t]) + B.part[2][t]) + B.part[3][t];
      gk = fmaf(ek, r, ak);
      dk = fabsf(gk - g);
      g = gk;
      B.gam[t] = gk;
      B.psi[t] = digamma_f32(gk);
    }
#pragma unroll
    for (int x = 1; x < oni::kWave; x <<= 1) {
      dk += __shfl_xor(dk, x);
      gk += __shfl_xor(gk, x);
    }
    if (lane == 0) {
      B.chg[wave] = dk;
      B.tot[wave] = gk;
    }
    __syncthreads();
    if (t == 0) {
      const float change = ((B.chg[0] + B.chg[1]) + B.chg[2]) + B.chg[3];
      const float total = ((B.tot[0] + B.tot[1]) + B.tot[2]) + B.tot[3];
      B.stop = change <= a.tol * total ? 1 : 0;
    }
    __syncthreads();
    ++nit;
    if (B.stop != 0) break;  // one word, the same for all 256 threads
  }
  float sum = 0.f;
#pragma unroll
  for (int kk = 0; kk < KQ; ++kk) {
    const int k = lane + kk * oni::kWave;
    if (k < K) sum += B.gam[k];
  }
#pragma unroll
  for (int x = 1; x < oni::kWave; x <<= 1) sum += __shfl_xor(sum, x);
  if (t < KS && t < KSMAX) {
    a.theta[d * KS + t] = t < K ? g / sum : 0.f;
    a.gamma[d * KS + t] = g;
  }
  if (t == 0) a.n_it[d] = nit;
  __syncthreads();  // gam / psi / e / red / stop are reused by the block's next document
}

template <int KSMAX, bool STAGE>
__global__ __launch_bounds__(kBlock) void k_vfold_exit(const VfoldExitArgs a) {
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
  for (;;) {  // the wave's rounds: wave_sync() only, no block barrier in here
    // the wave's next round (wave-uniform): skip what the block path takes, then the longest run
    // of documents whose pairs fit the tile
    while (s0 < nd && L.ptr[s0 + 1] - L.ptr[s0] > kTile) {
      if (lane == 0) L.big[nbig] = s0;
      ++nbig;
      ++s0;
    }
    int s1 = s0;
    while (s1 < nd && L.ptr[s1 + 1] - L.ptr[s0] <= kTile) ++s1;
    if (s1 == s0) break;  // s0 == nd: this wave has no round left
    const int ns = s1 - s0, items = ns * KS;
    const int64_t p0 = (int64_t)L.ptr[s0];
    const int np = (int)(L.ptr[s1] - p0);
    int word = 0, cnt = 0, myslot = s0;
    if (lane < np) {
      word = a.pair_word[p0 + lane];
      cnt = a.pair_cnt[p0 + lane];
      L.word[lane] = word;
      L.cnt[lane] = cnt;
      for (int s = s0 + 1; s < s1; ++s) myslot += L.ptr[s] <= p0 + lane ? 1 : 0;
    }
    wave_sync();
    if constexpr (STAGE) {
      for (int i = lane; i < np * KS4; i += oni::kWave) {
        const int r = i / KS4, c = (i - r * KS4) * 4;
        *reinterpret_cast<float4*>(L.rows + r * stride + c) =
            *reinterpret_cast<const float4*>(a.table + (int64_t)L.word[r] * KS + c);
      }
    }
    // γ0: the given rows by 16-byte loads, or a + N_d / K; the padding columns of both buffers are zero
    if (a.gamma0 != nullptr) {
      for (int i = lane; i < ns * KS4; i += oni::kWave) {
        const int r = i / KS4, c = (i - r * KS4) * 4;
        *reinterpret_cast<float4*>(L.gam + (s0 + r) * KS + c) = gamma0_at(a, d0 + s0 + r, c);
        *reinterpret_cast<float4*>(L.buf + (s0 + r) * KS + c) = make_float4(0.f, 0.f, 0.f, 0.f);
      }
    } else {
      for (int i = lane; i < items; i += oni::kWave) {
        const int sl = s0 + (int)__umulhi((uint32_t)i, ks_inv), k = i - (sl - s0) * KS;
        float v = 0.f;
        if (k < K) {
          const int lo = (int)(L.ptr[sl] - p0), hi = (int)(L.ptr[sl + 1] - p0);
          long long N = 0;
          for (int p = lo; p < hi; ++p) N += L.cnt[p];
          v = prior_at(a, d0 + sl, k) + (float)N / (float)K;
        }
        L.gam[sl * KS + k] = v;
        L.buf[sl * KS + k] = 0.f;
      }
    }
    const int rsl = s0 + (lane >> 2), rq = lane & 3;  // four lanes per document for max ψ, Σ|Δ| and Σγ
    const bool lead = rsl < s1 && rq == 0;
    bool live = lead && a.max_iters > 0;  // quad lane 0: its document still iterates
    int nit = 0;
    if (lead) L.act[rsl] = live ? 1 : 0;
    wave_sync();
    for (int it = 0; it < a.max_iters; ++it) {
      for (int i = lane; i < items; i += oni::kWave) {
        const int sl = s0 + (int)__umulhi((uint32_t)i, ks_inv), k = i - (sl - s0) * KS;
        if (k < K && L.act[sl] != 0) L.buf[sl * KS + k] = digamma_f32(L.gam[sl * KS + k]);
      }
      wave_sync();
      const bool ract = rsl < s1 && L.act[rsl] != 0;
      float m = -__builtin_inff();
      if (ract)
        for (int k = rq; k < K; k += 4) m = fmaxf(m, L.buf[rsl * KS + k]);
      m = fmaxf(m, __shfl_xor(m, 1));
      m = fmaxf(m, __shfl_xor(m, 2));
      if (ract && rq == 0) L.red[rsl] = m;
      wave_sync();
      for (int i = lane; i < items; i += oni::kWave) {
        const int sl = s0 + (int)__umulhi((uint32_t)i, ks_inv), k = i - (sl - s0) * KS;
        if (k < K && L.act[sl] != 0) L.buf[sl * KS + k] = expf(L.buf[sl * KS + k] - L.red[sl]);
      }
      wave_sync();
      if (lane < np && L.act[myslot] != 0) {  // lane = pair
        const float* row = STAGE ? L.rows + lane * stride : a.table + (int64_t)word * KS;
        L.q[lane] = (float)cnt / dot_e(row, L.buf + myslot * KS, KS);
      }
      wave_sync();
      for (int i = lane; i < items; i += oni::kWave) {  // lane = (document, k)
        const int sl = s0 + (int)__umulhi((uint32_t)i, ks_inv), k = i - (sl - s0) * KS;
        if (k < K && L.act[sl] != 0) {
          const int lo = (int)(L.ptr[sl] - p0), hi = (int)(L.ptr[sl + 1] - p0);
          float r = 0.f;
          for (int p = lo; p < hi; ++p) {
            const float x = STAGE ? L.rows[p * stride + k] : a.table[(int64_t)L.word[p] * KS + k];
            r = fmaf(L.q[p], x, r);
          }
          const float g = fmaf(L.buf[sl * KS + k], r, prior_at(a, d0 + sl, k));
          L.buf[sl * KS + k] = fabsf(g - L.gam[sl * KS + k]);
          L.gam[sl * KS + k] = g;
        }
      }
      wave_sync();
      float change = 0.f, total = 0.f;
      if (ract)
        for (int k = rq; k < K; k += 4) {
          change += L.buf[rsl * KS + k];
          total += L.gam[rsl * KS + k];
        }
      change += __shfl_xor(change, 1);
      total += __shfl_xor(total, 1);
      change += __shfl_xor(change, 2);
      total += __shfl_xor(total, 2);
      if (live) {
        ++nit;
        if (change <= a.tol * total) {
          live = false;
          L.act[rsl] = 0;
        }
      }
      const bool any = __ballot(live) != 0;  // wave-uniform
      wave_sync();
      if (!any) break;
    }
    float sum = 0.f;
    if (rsl < s1)
      for (int k = rq; k < K; k += 4) sum += L.gam[rsl * KS + k];
    sum += __shfl_xor(sum, 1);
    sum += __shfl_xor(sum, 2);
    if (lead) {
      L.red[rsl] = sum;
      a.n_it[d0 + rsl] = nit;
    }
    wave_sync();
    for (int i = lane; i < items; i += oni::kWave) {
      const int sl = s0 + (int)__umulhi((uint32_t)i, ks_inv), k = i - (sl - s0) * KS;
      const float g = L.gam[sl * KS + k];  // 0 in the padding columns
      const int64_t o = (d0 + sl) * KS + k;
      a.theta[o] = k < K ? g / L.red[sl] : 0.f;
      a.gamma[o] = g;
    }
    wave_sync();  // the next round reuses the wave's buffers
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

// oni_vfold's arguments with iters → max_iters, plus tol (finite, ≥ 0), gamma0 f32 [D][KS] or null
// (the cold start) and n_it_out int32 [D]; gamma_out is always written. Row widths up to 256.
ONI_API int oni_vfold_exit(const int32_t* pair_word, const int32_t* pair_cnt, const int64_t* doc_pair_ptr, int64_t D,
                           const float* table, int KS, int K, float alpha, const float* prior, int max_iters,
                           float tol, const float* gamma0, float* theta_out, float* gamma_out, int32_t* n_it_out,
                           hipStream_t s) {
  if (K < 1 || K > KS || KS % 4 != 0 || KS > 256 || max_iters < 0 || D < 0 || D > 0x7FFFFFFFll * 32) return (int)hipErrorInvalidValue;
  if (!(tol >= 0.f) || tol > 3.0e38f) return (int)hipErrorInvalidValue;
  if (D == 0) return 0;
  if (doc_pair_ptr == nullptr || table == nullptr || theta_out == nullptr || gamma_out == nullptr || n_it_out == nullptr) return (int)hipErrorInvalidValue;
  if (prior == nullptr && !(alpha > 0.f)) return (int)hipErrorInvalidValue;
  const VfoldExitArgs a{pair_word, pair_cnt, doc_pair_ptr, table, prior, gamma0, theta_out, gamma_out, n_it_out, D, KS, K, max_iters, alpha, tol};
  const unsigned grid = (unsigned)((D + kWaves * kSlots - 1) / (kWaves * kSlots));
  if (KS <= 32) k_vfold_exit<32, true><<<grid, kBlock, 0, s>>>(a);
  else if (KS <= 64) k_vfold_exit<64, true><<<grid, kBlock, 0, s>>>(a);
  else if (KS <= 128) k_vfold_exit<128, false><<<grid, kBlock, 0, s>>>(a);
  else k_vfold_exit<256, false><<<grid, kBlock, 0, s>>>(a);
  return (int)hipGetLastError();
}
