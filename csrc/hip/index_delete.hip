// Point deletion by tombstone: a deleted row is zeroed in every slab that holds it and its bit is
// set in a persistent bitmap `dead`, packed as a RowMask is (index_filter.hip): bit r % 64 of
// 64-bit word r / 64.
//
// Why zeroing keeps every unmasked search route exact without teaching it about the bitmap:
//  * a zero row scores exactly 0 in every scan (bf16, e4m3) and in every pruning image (the
//    quantisers guard amax > 0, so a zero row quantises to a zero image; the tracked bounds only
//    grow, so every pruning bound stays valid);
//  * each route stays exact over the PHYSICAL rows, zero rows included, and if the top-k over a
//    superset holds no dead row it is the top-k over the live rows.  So after any route,
//    results_dead_kernel tests the returned [NQ, k] row ids against `dead` and counts the hits
//    into a device flag.  Zero hits -- the only outcome while every query has at least k live rows
//    scoring above 0 -- means the result is exact as it stands;
//  * a hit gates (on the device, nothing read back) the exact masked list scan under the live
//    mask ~dead, whose launches exit at once while the flag is 0.
#include "common.h"

#include <algorithm>

namespace symb {

constexpr int TS_THREADS = 256;   // 4 waves = 4 rows per workgroup

// Zero one row of `bytes` bytes (a multiple of 8, the host checks) with a wave: 16-byte stores,
// or 8-byte ones where the row pitch is an odd multiple of 8 (1-byte elements at D % 16 == 8),
// whose odd rows start 8 bytes off a 16-byte boundary.
__device__ __forceinline__ void zero_row(char* p, int bytes, int lane) {
  if ((bytes & 15) == 0) {
    uint4* q = reinterpret_cast<uint4*>(p);
    for (int c = lane; c < bytes / 16; c += 64) q[c] = make_uint4(0u, 0u, 0u, 0u);
  } else {
    uint2* q = reinterpret_cast<uint2*>(p);
    for (int c = lane; c < bytes / 8; c += 64) q[c] = make_uint2(0u, 0u);
  }
}

// One wave per list entry: 16-byte zero stores over the row in `slab0` (and `slab1` when present),
// then lane 0 sets the row's bit.  Entries outside [0, n_valid) are skipped.  The list holds
// distinct rows; a row already dead is written again with the same bytes and the same bit.
__global__ __launch_bounds__(TS_THREADS) void tombstone_rows_kernel(
    const int* __restrict__ rows, int n, int n_valid, char* __restrict__ slab0, int row_bytes0,
    char* __restrict__ slab1, int row_bytes1, unsigned long long* __restrict__ dead) {
  const int lane = threadIdx.x & 63;
  const int e = (int)blockIdx.x * (TS_THREADS / 64) + ((int)threadIdx.x >> 6);
  if (e >= n) return;
  const int r = rows[e];
  if (r < 0 || r >= n_valid) return;
  zero_row(slab0 + (size_t)r * row_bytes0, row_bytes0, lane);
  if (slab1 != nullptr) zero_row(slab1 + (size_t)r * row_bytes1, row_bytes1, lane);
  if (lane == 0) atomicOr(dead + (r >> 6), 1ull << (r & 63));
}

// *hits += |{ i : ids[i] >= 0 and row ids[i] is dead }| (the caller zeroes *hits).  -1 ids (empty
// result slots) and ids past the bitmap are skipped.
__global__ __launch_bounds__(256) void results_dead_kernel(
    const int* __restrict__ ids, int n, const unsigned long long* __restrict__ dead, int n_words,
    int* __restrict__ hits) {
  int c = 0;
  for (int i = (int)(blockIdx.x * blockDim.x + threadIdx.x); i < n;
       i += (int)(gridDim.x * blockDim.x)) {
    const int r = ids[i];
    if (r >= 0 && (r >> 6) < n_words) c += (int)((dead[r >> 6] >> (r & 63)) & 1ull);
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) c += __shfl_xor(c, m, 64);
  if ((threadIdx.x & 63) == 0 && c != 0) atomicAdd(hits, c);
}

}  // namespace symb

using namespace symb;

// rows: [n] distinct ints on the device; slab0 / slab1 (slab1 may be null): [>= n_valid, D] of
// es0 / es1 bytes per element (2 or 1), D a multiple of 8; dead: [>= ceil(n_valid / 64)]
// 64-bit words.
int symb_tombstone_rows(const int* rows, int n, int n_valid, void* slab0, int es0, void* slab1,
                        int es1, int D, void* dead, hipStream_t st) {
  if (n <= 0) return 0;
  if (!rows || !slab0 || !dead || n_valid < 0 || D <= 0) return -1;
  if ((es0 != 1 && es0 != 2) || D % 8 != 0) return -1;
  if (slab1 && ((es1 != 1 && es1 != 2))) return -1;
  const int wpb = TS_THREADS / 64;
  hipLaunchKernelGGL(tombstone_rows_kernel, dim3((n + wpb - 1) / wpb), dim3(TS_THREADS), 0, st,
                     rows, n, n_valid, (char*)slab0, D * es0, (char*)slab1, slab1 ? D * es1 : 0,
                     (unsigned long long*)dead);
  return (int)hipGetLastError();
}

// ids: [n] ints (a search's [NQ, k] rows); dead: [n_words] 64-bit words; hits: one zeroed int.
int symb_results_dead(const int* ids, int n, const void* dead, int n_words, int* hits,
                      hipStream_t st) {
  if (n <= 0) return 0;
  if (!ids || !dead || !hits || n_words < 0) return -1;
  const int grid = std::max(1, std::min(64, (n + 255) / 256));
  hipLaunchKernelGGL(results_dead_kernel, dim3(grid), dim3(256), 0, st, ids, n,
                     (const unsigned long long*)dead, n_words, hits);
  return (int)hipGetLastError();
}
