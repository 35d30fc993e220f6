// In-place compaction of tombstoned rows: the live rows of a slab move down over the dead ones,
// driven by the packed `dead` bitmap (index_delete.hip: bit r % 64 of 64-bit word r / 64) and by
// `tile_dst`, the exclusive prefix over 64-row tiles of the live rows per tile (tile_dst[t] = the
// new row of tile t's first live row), which the host plans (index/shard.py compact_plan).
//
// One launch moves one WINDOW of source tiles [t0, t1), in one of two modes the plan chooses so
// that no workgroup ever has to wait on another:
//  * direct: every destination row of the window lies below every source row of the window
//    (tile_dst[t1] <= 64 t0), so the waves write straight into the slab in any order;
//  * staged: the live rows are gathered into a staging buffer at row tile_dst[t] - tile_dst[t0]
//    + rank, and the host enqueues one contiguous copy to rows [tile_dst[t0], tile_dst[t1])
//    behind the launch.
// Stream order between windows is the only synchronisation: no flags, no grid barrier, no spin.
#include "common.h"

namespace symb {

constexpr int CP_THREADS = 256;   // 4 waves = 4 source tiles per workgroup
constexpr int CP_UNROLL = 4;      // chunks in flight per lane (move_tile spells them out)

// Position of the r-th (0-based) set bit of `m`; r < popcount(m).
__device__ __forceinline__ int nth_set_bit(unsigned long long m, int r) {
  int pos = 0;
#pragma unroll
  for (int w = 32; w >= 1; w >>= 1) {
    const int c = __popcll((m >> pos) & ((1ull << w) - 1ull));
    if (r >= c) {
      r -= c;
      pos += w;
    }
  }
  return pos;
}

// The live rows of one tile, `bytes` bytes each (a multiple of sizeof(V)), copied by one wave in
// chunks of V: item i = (rank, chunk) flattened over the lanes, so a row of fewer than 64 chunks
// (768 bytes = 48 uint4) idles no lane.  Row `rank` of the tile's live rows goes from source row
// src_tile + (its bit) * bytes to dst + rank * bytes.
template <typename V>
__device__ __forceinline__ void move_tile(const char* src_tile, char* dst, int bytes,
                                          unsigned long long live, int n_live, int lane) {
  const int C = bytes / (int)sizeof(V);
  const int items = n_live * C;
  const int dq = 64 / C, dr = 64 % C;
  int rank = lane / C, chunk = lane % C;
  // CP_UNROLL (4) items per lane and trip, every load ahead of the first store; named scalars,
  // not arrays, so everything stays in registers
  for (int i0 = lane; i0 < items; i0 += 64 * CP_UNROLL) {
    const V* s0 = nullptr; const V* s1 = nullptr; const V* s2 = nullptr; const V* s3 = nullptr;
    V* d0 = nullptr; V* d1 = nullptr; V* d2 = nullptr; V* d3 = nullptr;
#define CP_ITEM(u, S, Dp)                                                                  \
    if (i0 + 64 * u < items) {                                                             \
      S = reinterpret_cast<const V*>(src_tile + (size_t)nth_set_bit(live, rank) * bytes) + chunk; \
      Dp = reinterpret_cast<V*>(dst + (size_t)rank * bytes) + chunk;                       \
    }                                                                                      \
    rank += dq;                                                                            \
    chunk += dr;                                                                           \
    if (chunk >= C) {                                                                      \
      chunk -= C;                                                                          \
      ++rank;                                                                              \
    }
    CP_ITEM(0, s0, d0)
    CP_ITEM(1, s1, d1)
    CP_ITEM(2, s2, d2)
    CP_ITEM(3, s3, d3)
#undef CP_ITEM
    V v0 = {}, v1 = {}, v2 = {}, v3 = {};
    if (s0) v0 = *s0;
    if (s1) v1 = *s1;
    if (s2) v2 = *s2;
    if (s3) v3 = *s3;
    if (d0) *d0 = v0;
    if (d1) *d1 = v1;
    if (d2) *d2 = v2;
    if (d3) *d3 = v3;
  }
}

__device__ __forceinline__ void move_tile_any(const char* src_tile, char* dst, int bytes,
                                              unsigned long long live, int n_live, int lane) {
  // 16-byte chunks, or 8-byte ones where the row pitch is an odd multiple of 8 (zero_row,
  // index_delete.hip)
  if ((bytes & 15) == 0)
    move_tile<uint4>(src_tile, dst, bytes, live, n_live, lane);
  else
    move_tile<uint2>(src_tile, dst, bytes, live, n_live, lane);
}

// One wave per source tile t in [t0, t1).  stage0 == nullptr: direct mode.  The slabs are read and
// (in direct mode) written through the same pointer, so nothing here is __restrict__.
// Guards on the device values (tile_dst comes from the host's plan, the bitmap from the shard):
// a tile whose destination would leave the slab / the staging capacity, or (direct) would not lie
// at or below its source, is not moved.
__global__ __launch_bounds__(CP_THREADS) void compact_rows_kernel(
    const unsigned long long* dead, const int* tile_dst, int t0, int t1, int n_valid, char* slab0,
    int row_bytes0, char* stage0, char* slab1, int row_bytes1, char* stage1, int stage_cap) {
  const int lane = threadIdx.x & 63;
  const int t = t0 + (int)blockIdx.x * (CP_THREADS / 64) + ((int)threadIdx.x >> 6);
  if (t >= t1) return;
  const int row0 = t * 64;
  const int valid = n_valid - row0;                 // rows of this tile below n_valid
  if (valid <= 0) return;
  unsigned long long live = ~dead[t];
  if (valid < 64) live &= (1ull << valid) - 1ull;
  const int n_live = __popcll(live);
  if (n_live == 0) return;
  const int d = tile_dst[t];
  if (stage0 == nullptr) {
    if (d < 0 || d > row0) return;
    if (d == row0) {
      // no dead row below this tile: the live rows below its first dead row stay where they are
      // (every row below the first dead bit is live, so that bit's position is their count; a
      // later row lands on the source of a row of LOWER rank only, which this wave has read)
      const int keep = n_live == 64 ? 64 : __ffsll(~live) - 1;
      const unsigned long long rest = keep < 64 ? live & ~((1ull << keep) - 1ull) : 0ull;
      const int n_rest = n_live - keep;
      if (n_rest <= 0) return;
      move_tile_any(slab0 + (size_t)row0 * row_bytes0,
                    slab0 + (size_t)(d + keep) * row_bytes0, row_bytes0, rest, n_rest, lane);
      if (slab1 != nullptr)
        move_tile_any(slab1 + (size_t)row0 * row_bytes1,
                      slab1 + (size_t)(d + keep) * row_bytes1, row_bytes1, rest, n_rest, lane);
      return;
    }
    move_tile_any(slab0 + (size_t)row0 * row_bytes0, slab0 + (size_t)d * row_bytes0, row_bytes0,
                  live, n_live, lane);
    if (slab1 != nullptr)
      move_tile_any(slab1 + (size_t)row0 * row_bytes1, slab1 + (size_t)d * row_bytes1,
                    row_bytes1, live, n_live, lane);
    return;
  }
  const int rel = d - tile_dst[t0];
  if (rel < 0 || rel + n_live > stage_cap) return;
  move_tile_any(slab0 + (size_t)row0 * row_bytes0, stage0 + (size_t)rel * row_bytes0, row_bytes0,
                live, n_live, lane);
  if (slab1 != nullptr)
    move_tile_any(slab1 + (size_t)row0 * row_bytes1, stage1 + (size_t)rel * row_bytes1,
                  row_bytes1, live, n_live, lane);
}

}  // namespace symb

using namespace symb;

// dead: [>= n_tiles] 64-bit words, tile_dst: [>= n_tiles + 1] ints (n_tiles = ceil(n_valid / 64)),
// both on the device; slab0 / slab1 (slab1 may be null): [>= n_valid, D] of es0 / es1 bytes per
// element (1 or 2), D a multiple of 8.  stage0 null: direct mode.  Otherwise stage0 (and stage1
// with slab1) hold `stage_cap` rows and the window gathers `n_rows` = tile_dst[t1] - tile_dst[t0]
// rows (the host's copy of the plan): -1 unless they fit.
int symb_compact_rows(const void* dead, const int* tile_dst, int t0, int t1, int n_valid,
                      void* slab0, int es0, void* stage0, void* slab1, int es1, void* stage1, int D,
                      int n_rows, int stage_cap, hipStream_t st) {
  if (!dead || !tile_dst || !slab0 || n_valid <= 0 || D <= 0) return -1;
  if ((es0 != 1 && es0 != 2) || D % 8 != 0) return -1;
  if (slab1 && es1 != 1 && es1 != 2) return -1;
  const int n_tiles = (n_valid + 63) / 64;
  if (t0 < 0 || t0 >= t1 || t1 > n_tiles) return -1;
  if (stage1 && !slab1) return -1;
  if (stage0) {
    if (slab1 && !stage1) return -1;
    if (n_rows < 0 || stage_cap < 0 || n_rows > stage_cap) return -1;
  } else if (stage1) {
    return -1;
  }
  // (a row pitch that is a multiple of 16 moves in 16-byte chunks, any other in 8-byte ones)
  for (const void* p : {(const void*)slab0, (const void*)stage0, (const void*)slab1,
                        (const void*)stage1})
    if ((uintptr_t)p % 16 != 0) return -1;
  const int wpb = CP_THREADS / 64;
  hipLaunchKernelGGL(compact_rows_kernel, dim3((t1 - t0 + wpb - 1) / wpb), dim3(CP_THREADS), 0, st,
                     (const unsigned long long*)dead, tile_dst, t0, t1, n_valid, (char*)slab0,
                     D * es0, (char*)stage0, (char*)slab1, slab1 ? D * es1 : 0, (char*)stage1,
                     stage0 ? stage_cap : 0);
  return (int)hipGetLastError();
}
