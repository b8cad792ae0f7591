// Fold-in inference (`lda inf`): doc-topic counts of new documents against a FROZEN word table.
//
// Replaces oni-lda-c's `lda inf` (lda-inference.c over a saved final.beta) for the
// Gibbs engine. A token of word w in doc d draws topic k with weight
//
//     p_k ∝ (n_dk^¬t + α) · φ_wk
//
// φ = the saved model's word table (row V: a word the model never saw), never updated. With φ
// frozen there is no cross-document dependency: no Δn_wk, no k_apply, no recount, no all-reduce.
// A chunk whose document is that one chunk therefore runs ALL sweeps of a launch back to back with
// its counts in registers (one read and one write of its n_dk row, whatever the sweep count), which
// no training sampler can do. Numerics are pinned and replayed bit for bit by
// oni355/ref/foldin_spec.py foldin_pass:
//
//   a_j = f32(n_j) + α at use; P_j = fma(a_j, φ_wj, P_{j−1}) along a lane's KP topics; lanes are
//   combined by the Hillis-Steele scan of the training samplers; z = min(#{P ≤ u·total}, K − 1).
//
// Draws: Philox4x32-10, counter (pos/4, doc key, sweep, stream) with stream 2 for the init pass
// (sweep 0) and 3 for the sweeps (training: 0 and 1).
//
// Execution model: as training, one unit of G lanes per chunk, a wave per SELL slice. Documents
// over several chunks need their chunks' Δ merged between sweeps: they are swept one sweep per
// launch (`select` 2, sweep-start row in ndk_src, Δ added into the pre-copied row of ndk_dst), and
// the host adds their window sums.
//
// Per-document priors (`prior`, the PRIOR instantiations): a document the saved model has a profile
// of draws from (n_dk^¬t + pr_dk)·φ_wk with pr_dk = α + m_d·θ^train_dk. A live unit loads its KP
// columns of the row once, before the sweeps, and forms a_j = f32(n_j) + pr_j at use; the rows are
// made by k_prior_rows below (oni355/ref/foldin_spec.py prior_rows).
#include "gibbs_sampler.h"

struct OniFoldin {
  const uint32_t* tok_word;    // SELL word ids (V = the out-of-vocabulary row)
  uint8_t* tok_z;              // SELL topics
  const int64_t* slice_off;    // [n_slices]
  const int32_t* slice_len;    // [n_slices]
  const int32_t* chunk_doc;    // [n_slices*S], -1 = padding chunk
  const int32_t* chunk_pos0;
  const uint32_t* chunk_key;
  const uint8_t* chunk_multi;
  const int32_t* ndk_src;      // [D][KS] sweep-start rows (sweeps)
  int32_t* ndk_dst;            // [D][KS]; may be ndk_src when no selected chunk is multi
  const float* phi;            // [V + 1][KS] frozen word table, columns ≥ K zero
  int32_t* ndk_sum;            // [D][KS] += the row after every sweep ≥ avg_from (single-chunk docs)
  int64_t n_slices;
  int32_t K;
  int32_t KS;
  float alpha;
  uint32_t seed0, seed1;
  int32_t sweep_lo;            // number of the first sweep of this launch (≥ 1)
  int32_t n_sweeps;            // sweeps run back to back (> 1: single-chunk chunks only)
  int32_t avg_from;            // first sweep whose rows enter ndk_sum
  int32_t select;              // 0 every chunk, 1 chunks of single-chunk docs, 2 chunks of multi-chunk docs
  const float* prior;          // [D][KS] per-document prior rows in α's place; nullptr = the flat prior α
};

namespace {

template <int G, int KP, bool INIT, bool PRIOR>
__global__ __launch_bounds__(kBlock) void k_foldin(const OniFoldin a) {
  constexpr int S = oni::kWave / G;
  constexpr int KS = G * KP;
  const int wave = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  const int c = lane / G;
  const int g = lane % G;
  const int kbase = g * KP;
  const int64_t slice = (int64_t)blockIdx.x * kWavesPerBlock + wave;
  if (slice >= a.n_slices) return;  // wave-uniform; the kernel has no block barrier
  const int64_t chunk = slice * S + c;
  // a chunk outside the launch's selection is a dead unit: neither live nor multi (no row of its
  // document is read or written)
  const int doc0 = a.chunk_doc[chunk];
  const bool multi0 = doc0 >= 0 && a.chunk_multi[chunk] != 0;
  const bool live = doc0 >= 0 && !((a.select == 1 && multi0) || (a.select == 2 && !multi0));
  const bool multi = live && multi0;
  const int doc = live ? doc0 : -1;
  if (!__ballot(live)) return;  // nothing selected in this slice
  const int len = a.slice_len[slice];
  const int64_t off = a.slice_off[slice];
  const uint32_t key = live ? a.chunk_key[chunk] : 0u;
  const uint32_t pos0 = live ? (uint32_t)a.chunk_pos0[chunk] : 0u;
  OniGibbs sd{};  // PhiloxPair reads only the seeds
  sd.seed0 = a.seed0;
  sd.seed1 = a.seed1;

  int32_t n[KP], acc[KP];
#pragma unroll
  for (int j = 0; j < KP; ++j) n[j] = acc[j] = 0;
  if (!INIT && live) load_row_i<KP>(a.ndk_src + (int64_t)doc * KS + kbase, n);
  float qv[KP];
#pragma unroll
  for (int j = 0; j < KP; ++j) qv[j] = 0.f;
  uint32_t wprev = oni::kPadWord;
  // the document's prior row (the same row in every chunk of a multi-chunk document); a dead unit
  // reads none and draws nothing
  float pr[PRIOR ? KP : 1];
  if constexpr (PRIOR) {
#pragma unroll
    for (int j = 0; j < KP; ++j) pr[j] = 0.f;
    if (live) load_row_f<KP>(a.prior + (int64_t)doc * KS + kbase, pr);
  }

  const int n_sweeps = INIT ? 1 : a.n_sweeps;
  for (int it = 0; it < n_sweeps; ++it) {
    const uint32_t sweep = INIT ? 0u : (uint32_t)(a.sweep_lo + it);
    PhiloxPair rng;
    rng.init(pos0, key, sweep, INIT ? 2u : 3u, sd);
    uint32_t w_nx = (live && len > 0) ? a.tok_word[off + c] : oni::kPadWord;
    int z_nx = (!INIT && live && len > 0) ? (int)a.tok_z[off + c] : 0;
    for (int s = 0; s < len; ++s) {
      const int64_t idx = off + (int64_t)s * S + c;
      const uint32_t w = w_nx;
      const int zo = z_nx;
      if (live && s + 1 < len) {
        w_nx = a.tok_word[idx + S];
        if (!INIT) z_nx = (int)a.tok_z[idx + S];
      }
      rng.step(s, sd);
      if (w == oni::kPadWord) continue;  // uniform across the G lanes of a unit
      const uint32_t rr = rng.pick(s);
      if constexpr (!INIT) {
#pragma unroll
        for (int j = 0; j < KP; ++j) n[j] -= (kbase + j == zo);
      }
      if (w != wprev) {
        load_row_f<KP>(a.phi + (int64_t)w * KS + kbase, qv);
        wprev = w;
      }
      float P[KP];
      float run = 0.f;
#pragma unroll
      for (int j = 0; j < KP; ++j) {
        float add;
        if constexpr (PRIOR) add = pr[j];
        else add = a.alpha;
        run = fmaf((float)n[j] + add, qv[j], run);
        P[j] = run;
      }
      float excl = 0.f, total = run;
      int cnt;
      if constexpr (G > 1) {
        const float incl = group_scan_dpp<G>(run, g);
        excl = dpp_row_shr<1>(incl);
        if (g == 0) excl = 0.f;
        total = __shfl(incl, G - 1, G);
        const float thr = oni::u01(rr) * total;
        cnt = group_sum_dpp<G>(count_le<KP>(P, excl, thr));
      } else {
        const float thr = oni::u01(rr) * total;
        cnt = count_le<KP>(P, 0.f, thr);
      }
      const int zn = cnt < a.K - 1 ? cnt : a.K - 1;
#pragma unroll
      for (int j = 0; j < KP; ++j) n[j] += (kbase + j == zn);
      // every lane of the unit stores the (same) topic: the next sweep of this launch then reads
      // back a byte the lane itself wrote -- program order, no fence between the sweeps
      if (INIT || zn != zo) a.tok_z[idx] = (uint8_t)zn;
    }
    if constexpr (!INIT) {
      if ((int)sweep >= a.avg_from) {
#pragma unroll
        for (int j = 0; j < KP; ++j) acc[j] += n[j];
      }
    }
  }

  // epilogue: a single-chunk doc stores its row (and adds its window sum), a multi-chunk doc adds Δ
  int32_t d[KP];
#pragma unroll
  for (int j = 0; j < KP; ++j) d[j] = 0;
  if (live && !multi) {
    int32_t* dst = a.ndk_dst + (int64_t)doc * KS + kbase;
#pragma unroll
    for (int j = 0; j < KP; j += 4) *reinterpret_cast<int4*>(dst + j) = make_int4(n[j], n[j + 1], n[j + 2], n[j + 3]);
    if (!INIT && a.sweep_lo + n_sweeps - 1 >= a.avg_from) {
      int32_t* sum = a.ndk_sum + (int64_t)doc * KS + kbase;
      int32_t s0[KP];
      load_row_i<KP>(sum, s0);
#pragma unroll
      for (int j = 0; j < KP; j += 4)
        *reinterpret_cast<int4*>(sum + j) =
            make_int4(s0[j] + acc[j], s0[j + 1] + acc[j + 1], s0[j + 2] + acc[j + 2], s0[j + 3] + acc[j + 3]);
    }
  }
  if (multi) {
    if constexpr (INIT) {
#pragma unroll
      for (int j = 0; j < KP; ++j) d[j] = n[j];
    } else {
      int32_t n0[KP];
      load_row_i<KP>(a.ndk_src + (int64_t)doc * KS + kbase, n0);
#pragma unroll
      for (int j = 0; j < KP; ++j) d[j] = n[j] - n0[j];
    }
  }
  if (__ballot(multi)) flush_multi_rows<G, KP>(a.ndk_dst, KS, doc, multi, kbase, d);
}

template <int G, int KP>
int launch_foldin(const OniFoldin& a, bool init, hipStream_t s) {
  if (a.KS != G * KP) return (int)hipErrorInvalidValue;
  const unsigned grid = (unsigned)((a.n_slices + kWavesPerBlock - 1) / kWavesPerBlock);
  if (grid == 0) return 0;
  if (a.prior != nullptr) {
    if (init) k_foldin<G, KP, true, true><<<grid, kBlock, 0, s>>>(a);
    else k_foldin<G, KP, false, true><<<grid, kBlock, 0, s>>>(a);
  } else {
    if (init) k_foldin<G, KP, true, false><<<grid, kBlock, 0, s>>>(a);
    else k_foldin<G, KP, false, false><<<grid, kBlock, 0, s>>>(a);
  }
  return (int)hipGetLastError();
}

// One thread per batch document: binary search of its key in the model's sorted keys, then its KS
// columns. m = min(f32(tokens), mass); pr_j = fma(m, θ_j, α) for j < K of a known document below
// the per-day IPv6 ids, α everywhere else.
constexpr int64_t kV6KeyBase = 0xF0000000ll;

__global__ __launch_bounds__(256) void k_prior_rows(const int64_t* __restrict__ mkeys, const float* __restrict__ mtheta,
                                                    const int64_t* __restrict__ mtokens, int64_t Dm,
                                                    const int64_t* __restrict__ keys, int64_t D, int K, int KS,
                                                    float alpha, float mass, float* __restrict__ out) {
  for (int64_t d = (int64_t)blockIdx.x * 256 + threadIdx.x; d < D; d += (int64_t)gridDim.x * 256) {
    const int64_t key = keys[d];
    int64_t lo = 0, hi = Dm;  // first model key ≥ key
    while (lo < hi) {
      const int64_t mid = lo + ((hi - lo) >> 1);
      if (mkeys[mid] < key) lo = mid + 1;
      else hi = mid;
    }
    const bool hit = lo < Dm && mkeys[lo] == key && key < kV6KeyBase;
    float* o = out + d * KS;
    if (hit) {
      const float tk = (float)mtokens[lo];
      const float m = tk < mass ? tk : mass;
      const float* th = mtheta + lo * K;
      for (int j = 0; j < K; ++j) o[j] = fmaf(m, th[j], alpha);
      for (int j = K; j < KS; ++j) o[j] = alpha;
    } else {
      for (int j = 0; j < KS; ++j) o[j] = alpha;
    }
  }
}

}  // namespace

// mkeys int64 [Dm] strictly ascending, mtheta f32 [Dm][K], mtokens int64 [Dm]; keys int64 [D]; out f32 [D][KS]
ONI_API int oni_prior_rows(const int64_t* mkeys, const float* mtheta, const int64_t* mtokens, int64_t Dm,
                           const int64_t* keys, int64_t D, int K, int KS, float alpha, float mass, float* out,
                           hipStream_t s) {
  if (K < 1 || K > KS || Dm < 0 || D < 0) return (int)hipErrorInvalidValue;
  if (D == 0) return 0;
  k_prior_rows<<<oni::grid_for(D, 256, 2048), 256, 0, s>>>(mkeys, mtheta, mtokens, Dm, keys, D, K, KS, alpha, mass, out);
  return (int)hipGetLastError();
}

ONI_API int oni_foldin_sizeof_args() { return (int)sizeof(OniFoldin); }

// The tilings of the training samplers: the ONI_TILINGS table of gibbs_sampler.h. Anything else
// (and a launch that would sweep a multi-chunk document more than once): hipErrorInvalidValue.
ONI_API int oni_foldin_launch(const OniFoldin* a, int G, int KP, int init, hipStream_t s) {
  if (a == nullptr || a->K < 1 || a->K > G * KP || a->K > 255 || a->select < 0 || a->select > 2) return (int)hipErrorInvalidValue;
  if (!init && (a->n_sweeps < 1 || a->sweep_lo < 1 || (a->n_sweeps > 1 && a->select != 1))) return (int)hipErrorInvalidValue;
#define ONI_FOLDIN_CASE(g_, kp_) \
  if (G == g_ && KP == kp_) return launch_foldin<g_, kp_>(*a, init != 0, s);
  ONI_TILINGS(ONI_FOLDIN_CASE)
#undef ONI_FOLDIN_CASE
  return (int)hipErrorInvalidValue;
}
