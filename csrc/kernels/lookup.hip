// oni355 -- lookup of every event's key in a saved, sorted table (k_table_lookup).
//
// Fold-in scoring maps each word key of the batch to its row of the saved model's vocabulary, and
// each proxy user-agent hash to its count in the model's frequency table: n queries (up to tens of
// millions) against M strictly ascending int64 keys (a few thousand to a few hundred thousand).
//
// A per-lane binary search over the table is log2(M) = 13-18 DEPENDENT global loads (L2 hit
// ~200 cycles each). Here every block first stages a coarse level of the table in LDS -- every
// stride-th key, stride = ceil(M / kSamples) -- and a query searches that level with LDS reads
// (~50 cycles each, the first steps wave-uniform broadcasts); only the last log2(stride) steps
// (2 for a 5.7k-key table, 7 for 194k keys) go to memory, and a query that equals a sample none.
//
// LDS budget: 8 blocks of 256 threads per CU (32 waves, the CU's cap) x 16 KiB = 128 KiB of the
// CU's 160 KiB, so the coarse level never limits occupancy: kSamples = 16 KiB / 8 B = 2048.
//
// Misses are counted per wave (ballot + popcount over the wave's queries of every round of the
// grid-stride loop) and added by one lane with ONE integer atomic per wave: integer sums, so the
// count is deterministic; the host reads it whenever it next reads results, never behind the lookup.
#include "oni_common.h"

namespace {

constexpr int kBlock = 256;
constexpr int kSamples = 2048;  // coarse level in LDS: 2048 x 8 B = 16 KiB per block
constexpr int64_t kI32Max = 0x7FFFFFFFll;

// VALUES = false (id mode): out[i] = position of queries[i] in keys, M on a miss.
// VALUES = true (value mode): out[i] = (int32)min(values[pos], 2^31 - 1), 0 on a miss.
template <bool VALUES>
__global__ __launch_bounds__(kBlock) void k_table_lookup(const int64_t* __restrict__ keys,
                                                         const int64_t* __restrict__ values, int64_t M,
                                                         const int64_t* __restrict__ queries, int64_t n,
                                                         int32_t* __restrict__ out,
                                                         unsigned long long* __restrict__ misses) {
  __shared__ int64_t coarse[kSamples];
  const int64_t stride = M > 0 ? (M + kSamples - 1) / kSamples : 1;
  const int S = (int)((M + stride - 1) / stride);  // samples: keys[0], keys[stride], ... (S <= kSamples)
  for (int j = threadIdx.x; j < S; j += kBlock) coarse[j] = keys[(int64_t)j * stride];
  __syncthreads();

  unsigned long long wave_miss = 0;  // the wave's misses so far (the same value on every lane)
  // every lane of a block runs the same number of rounds, so the ballot sees whole waves
  for (int64_t base = (int64_t)blockIdx.x * kBlock; base < n; base += (int64_t)gridDim.x * kBlock) {
    const int64_t i = base + threadIdx.x;
    const bool live = i < n;
    bool hit = false;
    int64_t pos = 0;
    if (live) {
      const int64_t q = queries[i];
      int lo = 0, hi = S;  // first sample > q
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (coarse[mid] <= q) lo = mid + 1;
        else hi = mid;
      }
      if (lo > 0) {  // keys[(lo-1)·stride] <= q < the next sample (or the table's end)
        const int64_t first = (int64_t)(lo - 1) * stride;
        if (coarse[lo - 1] == q) {
          hit = true;
          pos = first;
        } else {
          int64_t a = first + 1, b = first + stride < M ? first + stride : M;
          while (a < b) {
            const int64_t mid = a + ((b - a) >> 1);
            const int64_t v = keys[mid];
            if (v < q) {
              a = mid + 1;
            } else {
              b = mid;
              if (v == q) {  // strictly ascending keys: everything below mid is < q from here on
                hit = true;
                pos = mid;
              }
            }
          }
        }
      }
      if (VALUES) {
        int64_t v = 0;
        if (hit) {
          v = values[pos];
          v = v < kI32Max ? v : kI32Max;
        }
        out[i] = (int32_t)v;
      } else {
        out[i] = (int32_t)(hit ? pos : M);
      }
    }
    wave_miss += (unsigned long long)__popcll(__ballot(live && !hit));
  }
  if ((threadIdx.x & (oni::kWave - 1)) == 0 && wave_miss != 0) atomicAdd(misses, wave_miss);
}

}  // namespace

// keys int64 [M] strictly ascending (signed order), values int64 [M] or null (id mode), queries
// int64 [n], out int32 [n]; *misses (u64, device) is ADDED to, the caller zeroes it.
ONI_API int oni_table_lookup(const int64_t* keys, const int64_t* values, int64_t M, const int64_t* queries,
                             int64_t n, int32_t* out, unsigned long long* misses, hipStream_t s) {
  if (M < 0 || n < 0 || M > kI32Max || misses == nullptr) return (int)hipErrorInvalidValue;
  if (n == 0) return 0;
  if (out == nullptr || queries == nullptr || (M > 0 && keys == nullptr)) return (int)hipErrorInvalidValue;
  // 8 resident blocks on each of the 256 CUs: every block stages the coarse level once
  const unsigned grid = oni::grid_for(n, kBlock, 2048);
  if (values != nullptr) k_table_lookup<true><<<grid, kBlock, 0, s>>>(keys, values, M, queries, n, out, misses);
  else k_table_lookup<false><<<grid, kBlock, 0, s>>>(keys, values, M, queries, n, out, misses);
  return (int)hipGetLastError();
}
