// Exact top-k under a row mask over an fp8 (OCP e4m3) shard, one kernel for both mask forms:
// index_scan_fp8_kernel (index_fp8.hip) made to walk only the 64-row tiles that hold an allowed
// row and to ignore disallowed rows in them, the way index_scan_filter_kernel (index_filter.hip) is
// the masked form of the bf16 list scan.  Mask format, live-tile list (symb_filter_tiles) and
// candidate layout are that file's.  index_filter_fp8.hip instantiates GROUPED = false (one mask
// for every query), index_filter_group_fp8.hip GROUPED = true (a mask per query).
//
// From the fp8 scan: 4 waves, 64 queries per wave as two 32-query B-fragment sets resident in
// AGPRs, v_mfma_f32_32x32x64_f8f6f4 through Fp8Chain, the Fp8Swz LDS image, the LDS-DMA ring with
// counted vmcnt and a raw barrier, per-lane register top-k, candidates [NQ][n_rblk][2][kmax] of raw
// accumulators (S^2 * cosine; thr_init in the same units).  The per-row MFMA chain is unchanged
// and a column does not depend on its neighbours, so a row scores bit for bit what it scores in
// the unfiltered scan, under either mask form.
//
// From the bf16 masked scan: workgroup rb walks the slice [rb * per, min((rb + 1) * per, n_live))
// of the live-tile list, per = ceil(n_live / n_rblk), n_live read from device memory; `stride`
// walks every stride-th entry of the slice; the DMA source of a ring slot is
// X + (tile * 64 + half) * D with tile read from the list (a wave-uniform base beside the
// unchanged per-lane offsets); the tile's mask word, cut at n_valid by live_word, sends every
// accumulator whose row bit is clear to -inf before the max test (this replaces the unfiltered
// kernel's row_end test).  A list entry is a 64-row tile; a barrier interval is 32 * SUBS rows,
// i.e. one entry at SUBS = 2 and half of one at SUBS = 1 (D = 768), where the mask of t_nxt is
// loaded every interval and the interval's bits are w >> (h0 + sub * 32).
//
// Ring geometry: the unfiltered scan's (Fp8Cfg: NS = 6 / 5 / 4 / 6 / 2 at 256 / 384 / 512 / 768 /
// 1024), not a shallower one.  The ring's depth is what hides HBM latency behind the MFMA chains,
// and under a mask consecutive slots come from scattered tiles, which makes a load slower, not
// faster; the price of the depth is only that the prologue reads the list entries of the first
// NS intervals (one batch of NS scalar loads, waited for once) where the bf16 kernel reads two.
// After the prologue the scalar state does not depend on NS: t_cur = tile of interval t, t_nxt =
// tile of t + 1 (its mask is loaded one interval ahead), t_pf = tile of the interval prefetched
// during t (t + NS - 1).
//
// Every read of the list goes through tile_ptr, which clamps the interval to the slice's last
// walked one at the stride in use: the list is uninitialised past n_live, and an index read there
// would become a DMA address.  Re-loading the last interval when the slice is shorter than the
// ring (or at its tail) keeps the counted vmcnt exact.  Scalar loads are issued right after the
// barrier, before the interval's first ds_read, and waited for at its end (scan_common.h).
//
// What GROUPED changes is where the mask words come from and how they are applied; every such
// site is an `if constexpr` below.
//  - single mask: `mask` is uint64 [n_words], qgroup is null.  The tile's word comes by one
//    s_load_dwordx2 and stays in SGPRs (w0; w1 is unused); mask_rows clears both query sets
//    under the same wave-uniform bits.
//  - grouped (mask_group.h): `mask` is uint64 [n_words][8], slot g = group g's word; qgroup is
//    int32 [NQ], & 7; tiles / n_live = filter_tiles of the OR of the slots.  The eight words of
//    the NEXT tile come by one hand-issued s_load_dwordx16; the lane's words are picked by
//    compare-and-select chains, cut at n_valid (the cut is wave-uniform: the tile is), and only
//    the picked words cross the barrier.  A lane holds TWO queries, query0 (B set 0) and query1 =
//    query0 + 32 (set 1), which may belong to different groups: it carries two group ids (packed
//    into one VGPR) and two picked words w0 / w1 (VGPR pairs), and mask_rows sends set 0's
//    accumulators to -inf under w0's bits and set 1's under w1's.  The all-rows-allowed shortcut
//    is a wave vote over both sets (the reasons are index_filter_group.hip's); a lane whose bits
//    are full takes no select under either form, so the vote cannot change a score.
//  - grouped at kmax = 32 (LATE) places the load differently.  A top-k update at kmax = 32 holds
//    32 compare masks, 64 SGPRs, and the single-mask form already fills the SGPR file there;
//    sixteen more in flight across an update are spilled whatever the load is split into (x16,
//    2 x8 and 4 x4 gave the same counts).  So the words are loaded during the interval's LAST
//    MFMA chain -- issued at its start, waited for at its end, where every ds_read of the chain
//    is consumed and the wait is for scalar loads alone -- and picked right after the last
//    mask_rows, before the last two updates; the tile indices are waited for there too.  No
//    update runs with the words in flight.  Where the interval has two chains (SUBS = 2) the
//    tile's 64 bytes are touched by a one-dword scalar load at the barrier, so the x16 one chain
//    later finds them in the scalar cache; at SUBS = 1 the x16 is issued at the barrier as
//    everywhere else.
//
// Register budget: profiles/fold_masked_scans/README.md.  No instantiation uses scratch or
// spills a register.
#pragma once
#include "fp8_scan.h"
#include "mask_group.h"

namespace symb {

template <int D, int KMAX, int NS, int SUBS, int AUX, bool GROUPED>
__global__ __launch_bounds__(256, 1) void index_scan_filter_fp8_kernel(
    const uint8_t* __restrict__ X, int n_valid, const int* __restrict__ tiles,
    const int* __restrict__ n_live_p, const uint64_t* __restrict__ mask,
    const int* __restrict__ qgroup, int stride, const uint8_t* __restrict__ Q, int NQ, int n_qblk,
    int xcd, const float* __restrict__ thr_init, float* __restrict__ cand_s,
    int* __restrict__ cand_i, const int* __restrict__ gate) {
  // gate (optional): run only if *gate != 0 (index_filter.hip has the note)
  if (gate != nullptr && *gate == 0) return;
  constexpr int CPR = D / 16, SUB = 32, TR = 32 * SUBS, NW = 4;
  constexpr int IPE = 64 / TR;                     // barrier intervals per list entry
  constexpr int TILE_BYTES = TR * D, SUB_BYTES = SUB * D;
  constexpr int LOADS = TILE_BYTES / (1024 * NW);  // DMA pieces per wave per interval
  // fragment reads in flight: 4 as in the unfiltered scan; at D = 1024 the kmax = 32 lists beside
  // 256 AGPRs of queries leave room for 3 (at 4 that instantiation spills one VGPR to scratch),
  // and the grouped form takes one fewer at 256 / kmax 32 too (at 4 it spills four SGPRs)
  constexpr int NKS = D / 64;
  constexpr int PF = ((D == 1024 || (GROUPED && D == 256)) && KMAX > 16) ? 3 : 4, R = PF + 1;
  static_assert((D % 256 == 0 || D == 384) && TILE_BYTES % (1024 * NW) == 0, "fp8 scan geometry");
  static_assert(SUBS == 1 || SUBS == 2, "an interval is half a list entry or a whole one");
  using Swz = Fp8Swz<D>;
  constexpr int G = Swz::G;
  static_assert(NS >= 2 && NS * TILE_BYTES <= 160 * 1024, "LDS ring exceeds the CU's 160 KiB");
  static_assert(LOADS <= NKS, "DMA pieces must fit the first chain");
  static_assert(LOADS * (NS - 2) < 64, "vmcnt range");
  // grouped, kmax = 32: the sixteen SGPRs of the words in flight may not be live during a top-k
  // update, whose 32 compare masks already fill the SGPR file (header note)
  constexpr bool LATE = GROUPED && KMAX > 16;

  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lb = xcd ? xcd_remap(blockIdx.x, gridDim.x) : blockIdx.x;
  const int qb = lb % n_qblk, rb = lb / n_qblk;
  const int n_rblk = gridDim.x / n_qblk;
  const int h = lane >> 5;

  // ---- this workgroup's slice of the live-tile list ----
  const int n_live = __builtin_amdgcn_readfirstlane(*n_live_p);
  const int per = (n_live + n_rblk - 1) / n_rblk;
  const int slice_begin = __builtin_amdgcn_readfirstlane(min(rb * per, n_live));
  const int slice_len = min(per, n_live - slice_begin);
  const int n_ent = slice_len > 0 ? (slice_len + stride - 1) / stride : 0;   // entries walked
  const int n_iv = __builtin_amdgcn_readfirstlane(n_ent * IPE);              // barrier intervals
  // interval iv (clamped to the last one) -> its entry's position in the list / its first row
  // within that entry's tile.  Called with n_iv > 0 only.
  auto tile_ptr = [&](int iv) {
    return tiles + slice_begin + (min(iv, n_iv - 1) / IPE) * stride;
  };
  auto half_row = [&](int iv) { return (min(iv, n_iv - 1) % IPE) * TR; };

  const int query0 = qb * 256 + wave * 64 + (lane & 31);
  const int query1 = query0 + 32;
  i32x8 q0[NKS], q1[NKS];
  {
    const uint8_t* p0 = Q + (size_t)min(query0, NQ - 1) * D + h * 32;
    const uint8_t* p1 = Q + (size_t)min(query1, NQ - 1) * D + h * 32;
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) {
      q0[ks] = *reinterpret_cast<const i32x8*>(p0 + ks * 64);
      q1[ks] = *reinterpret_cast<const i32x8*>(p1 + ks * 64);
    }
  }
  // per-piece source offsets within an interval, as in index_scan_fp8_kernel
  constexpr int RPS = (NW * 64) % CPR == 0 ? NW * 64 / CPR : 0;   // rows per piece step
  constexpr int GP = (G == 16 && RPS > 0 && 16 % RPS == 0 && LOADS % (16 / RPS) == 0)
                         ? 16 / RPS : LOADS;
  uint32_t goff[GP];
#pragma unroll
  for (int i = 0; i < GP; ++i) {
    const int s = (i * NW + wave) * 64 + lane;  // 16-byte LDS slot this lane fills
    const int row = s / CPR, pc = s % CPR;
    goff[i] = (uint32_t)(row * D + (Swz::phys(pc, row) << 4));   // the swizzle is an involution
  }
  // row_base: first row of the interval (wave-uniform); slot: interval number (ring position)
  auto issue_piece = [&](int row_base, int slot, int i) {
    const uint8_t* base = X + (size_t)row_base * D;
    char* dst = smem + (slot % NS) * TILE_BYTES;
    glds16_aux<AUX>(base + (size_t)(i / GP) * (GP * RPS * D) + goff[i % GP],
                    dst + (i * NW + wave) * 1024);
  };
  const uint32_t lds_smem = lds_addr(smem);
  uint32_t voff[8];
  {
    const int r = lane & 31;
#pragma unroll
    for (int m = 0; m < G / 4; ++m)
#pragma unroll
      for (int j = 0; j < 2; ++j)
        voff[m * 2 + j] = (uint32_t)(r * D + (Swz::phys(4 * m + 2 * h + j, r) << 4));
  }

  float tv0[KMAX], tv1[KMAX];
  int ti0[KMAX], ti1[KMAX];
#pragma unroll
  for (int i = 0; i < KMAX; ++i) {
    tv0[i] = tv1[i] = -INFINITY;
    ti0[i] = ti1[i] = -1;
  }
  // thr_init[q] (optional): a lower bound on query q's final k-th ALLOWED score, raw units
  float thr0 = thr_init ? thr_init[min(query0, NQ - 1)] : -INFINITY;
  float thr1 = thr_init ? thr_init[min(query1, NQ - 1)] : -INFINITY;
  // grouped: the lane's two mask groups in one register, set 0's in bits 0-2 and set 1's in
  // bits 4-6 (padded lanes take the last query's, like its fragments)
  int grps = 0;
  if constexpr (GROUPED)
    grps = (qgroup[min(query0, NQ - 1)] & (MASK_GROUPS - 1)) |
           ((qgroup[min(query1, NQ - 1)] & (MASK_GROUPS - 1)) << 4);
  // grouped: the lane's two words out of a tile's eight, cut at n_valid
  auto pick2 = [&](const u32x16& w8, int tile, uint64_t& w0, uint64_t& w1) {
    const uint64_t cut = live_word(~0ull, tile, n_valid);
    // (opaque: the fourteen compares against the group ids are loop invariants, and hoisted
    // out of the interval loop their masks are 28 SGPRs held across it)
    int g = grps;
    asm volatile("" : "+v"(g));
    w0 = pick_word<true>(w8, g & 15) & cut;
    w1 = pick_word<true>(w8, g >> 4) & cut;
  };
  // row of accumulator register r within the 32-row sub-tile = 4 h + acc_reg_row(r), for both
  // query sets; b0 / b1: the sub-tile's 32 mask bits of the lane's set 0 / set 1 query, bit j =
  // row j allowed.  Single mask: b0 is wave-uniform and serves both sets.  Grouped: the
  // shortcut is a wave vote over both sets (header note).
  auto mask_rows = [&](f32x16& a0, f32x16& a1, uint32_t b0, uint32_t b1) {
    if constexpr (!GROUPED) {
      if (b0 != 0xffffffffu) {
        const uint32_t lbits = b0 >> (4 * h);
#pragma unroll
        for (int r = 0; r < 16; ++r)
          if (!((lbits >> acc_reg_row<true>(r)) & 1u)) {
            a0[r] = -INFINITY;
            a1[r] = -INFINITY;
          }
      }
    } else {
      if (__any(b0 != 0xffffffffu || b1 != 0xffffffffu)) {
        const uint32_t l0 = b0 >> (4 * h), l1 = b1 >> (4 * h);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          if (!((l0 >> acc_reg_row<true>(r)) & 1u)) a0[r] = -INFINITY;
          if (!((l1 >> acc_reg_row<true>(r)) & 1u)) a1[r] = -INFINITY;
        }
      }
    }
  };
  auto update = [&](f32x16& acc, float (&tv)[KMAX], int (&ti)[KMAX], float& thr, int row0) {
    const int rb4 = row0 + 4 * h;
    float mx = acc[0];
#pragma unroll
    for (int r = 1; r < 16; ++r) mx = fmaxf(mx, acc[r]);
    if (mx > thr) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        if (acc[r] > thr) {
          topk_insert_par<KMAX>(tv, ti, acc[r], rb4 + acc_reg_row<true>(r));
          thr = fmaxf(thr, tv[KMAX - 1]);
        }
      }
    }
  };

  // w0 (and, grouped, w1): mask word(s) of interval t's tile, cut at n_valid
  int t_cur = 0, t_nxt = 0, t_pf = 0;
  uint64_t w0 = 0, w1 = 0;
  if (n_iv > 0) {
    // tiles of intervals 0 .. NS - 1 (each clamped to the slice): 0 .. NS - 2 fill the ring now,
    // NS - 1 is interval 0's prefetch
    int tp[NS];
#pragma unroll
    for (int p = 0; p < NS; ++p) sload_i32(tp[p], tile_ptr(p));
    swait_n<NS>(tp);
    t_cur = tp[0];
    t_nxt = tp[1];
    t_pf = tp[NS - 1];
    if constexpr (GROUPED) {
      u32x16 w8;
      sload_mask8(w8, mask + (size_t)MASK_GROUPS * t_cur);
      swait_mask8(t_cur, t_nxt, w8);
      pick2(w8, t_cur, w0, w1);
    } else {
      sload_u64(w0, mask + t_cur);
      swait(t_cur, t_nxt, w0);
      w0 = live_word(w0, t_cur, n_valid);
    }
#pragma unroll
    for (int p = 0; p < NS - 1; ++p) {
      const int row_base = tp[p] * 64 + half_row(p);
#pragma unroll
      for (int i = 0; i < LOADS; ++i) issue_piece(row_base, p, i);
    }
  }
  i32x4 lo[R], hi[R];
  for (int t = 0; t < n_iv; ++t) {
    // interval t landed for this wave once only the (NS-2) younger intervals' loads remain
    wait_vmcnt<LOADS * (NS - 2)>();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    // next interval's scalar state (waited for at the end of this interval; LATE: below)
    int n_nxt, n_pf, warm = 0;
    uint64_t n_w;
    u32x16 n_w8;
    sload_i32(n_nxt, tile_ptr(t + 2));
    sload_i32(n_pf, tile_ptr(t + NS));
    if constexpr (!GROUPED)
      sload_u64(n_w, mask + t_nxt);
    else if constexpr (!LATE || SUBS == 1)
      sload_mask8(n_w8, mask + (size_t)MASK_GROUPS * t_nxt);
    else   // one dword of the 64 bytes: the line is in the scalar cache when the x16 asks
      sload_i32(warm, reinterpret_cast<const int*>(mask + (size_t)MASK_GROUPS * t_nxt));

    const uint32_t tbase = lds_smem + (uint32_t)((t % NS) * TILE_BYTES);
    const int h0 = half_row(t);
    const int row0 = t_cur * 64 + h0;
    const int pf_row = t_pf * 64 + half_row(t + NS - 1);
    const int tnext = t + NS - 1;
    auto dma = [&](int i) { issue_piece(pf_row, tnext, i); };
#pragma unroll
    for (int sub = 0; sub < SUBS; ++sub) {
      const uint32_t base = tbase + sub * SUB_BYTES;
      f32x16 acc0, acc1;
      if constexpr (LATE && SUBS > 1)
        if (sub == SUBS - 1) sload_mask8(n_w8, mask + (size_t)MASK_GROUPS * t_nxt);
      if (sub == 0) {
        fp8_prologue<0, PF, R, G>(lo, hi, voff, base);
        Fp8Chain<0, NKS, PF, LOADS, G>::run(acc0, acc1, lo, hi, q0, q1, voff, base, dma);
      } else {
        Fp8Chain<0, NKS, PF, 0, G>::run(acc0, acc1, lo, hi, q0, q1, voff, base, NoDma());
      }
      if (sub + 1 < SUBS)  // next sub-tile's first fragments fly during this top-k
        fp8_prologue<0, PF, R, G>(lo, hi, voff, base + SUB_BYTES);
      // (reads of the asm MFMA results stay below the chain-end s_nops: index_i8.hip emit)
      asm volatile("" : "+v"(acc0), "+v"(acc1));
      mask_rows(acc0, acc1, (uint32_t)(w0 >> (h0 + sub * SUB)), (uint32_t)(w1 >> (h0 + sub * SUB)));
      if constexpr (LATE)
        if (sub == SUBS - 1) {   // the chain's ds_reads are consumed: only scalar loads are out
          swait_mask8(n_nxt, n_pf, n_w8);
          asm volatile("" : "+s"(warm));
          pick2(n_w8, t_nxt, w0, w1);
        }
      update(acc0, tv0, ti0, thr0, row0 + sub * SUB);
      update(acc1, tv1, ti1, thr1, row0 + sub * SUB);
    }

    if constexpr (!GROUPED) {
      swait(n_nxt, n_pf, n_w);
    } else if constexpr (!LATE) {
      swait_mask8(n_nxt, n_pf, n_w8);
      pick2(n_w8, t_nxt, w0, w1);
    }
    t_cur = t_nxt;
    t_nxt = n_nxt;
    t_pf = n_pf;
    if constexpr (!GROUPED) w0 = live_word(n_w, t_cur, n_valid);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // drain the tail prefetches before exit

  if (query0 < NQ) {
    const size_t base = (((size_t)query0 * n_rblk + rb) * 2 + h) * KMAX;
#pragma unroll
    for (int i = 0; i < KMAX; ++i) {
      cand_s[base + i] = tv0[i];
      cand_i[base + i] = ti0[i];
    }
  }
  if (query1 < NQ) {
    const size_t base = (((size_t)query1 * n_rblk + rb) * 2 + h) * KMAX;
#pragma unroll
    for (int i = 0; i < KMAX; ++i) {
      cand_s[base + i] = tv1[i];
      cand_i[base + i] = ti1[i];
    }
  }
}

template <bool GROUPED, int D, int KMAX, int AUX>
static int launch_filter_fp8(const void* X, int n_valid, const int* tiles, const int* n_live,
                             const void* mask, const int* qgroup, int stride, int n_rblk,
                             const void* Q, int NQ, int n_qblk, int xcd, const float* thr,
                             float* cs, int* ci, hipStream_t st, const int* gate) {
  constexpr int SUBS = Fp8Cfg<D>::SUBS, NS = Fp8Cfg<D>::NS;
  auto kern = index_scan_filter_fp8_kernel<D, KMAX, NS, SUBS, AUX, GROUPED>;
  constexpr int lds = NS * 32 * SUBS * D;
  set_max_lds<index_scan_filter_fp8_kernel<D, KMAX, NS, SUBS, AUX, GROUPED>>(lds);
  hipLaunchKernelGGL(kern, dim3(n_rblk * n_qblk), dim3(256), lds, st, (const uint8_t*)X, n_valid,
                     tiles, n_live, (const uint64_t*)mask, qgroup, stride, (const uint8_t*)Q, NQ,
                     n_qblk, xcd, thr, cs, ci, gate);
  return (int)hipGetLastError();
}

template <bool GROUPED, int D>
static int filter_fp8_dispatch(int kmax, int aux, const void* X, int n_valid, const int* tiles,
                               const int* n_live, const void* mask, const int* qgroup, int stride,
                               int n_rblk, const void* Q, int NQ, int n_qblk, int xcd,
                               const float* thr, float* cs, int* ci, hipStream_t st,
                               const int* gate) {
#define SYMB_L(K, A) launch_filter_fp8<GROUPED, D, K, A>(X, n_valid, tiles, n_live, mask, qgroup, stride, n_rblk, Q, NQ, n_qblk, xcd, thr, cs, ci, st, gate)
  if (kmax == 16) return aux ? SYMB_L(16, 2) : SYMB_L(16, 0);
  return aux ? SYMB_L(32, 2) : SYMB_L(32, 0);
#undef SYMB_L
}

// The body of both entry points: argument checks, then the width switch.  qgroup is required
// when GROUPED and ignored (pass null) otherwise.
template <bool GROUPED>
static int index_scan_filter_fp8(const void* X, int n_valid, int D, const int* tiles,
                                 const int* n_live, const void* mask, const int* qgroup,
                                 int stride, int n_rblk, const void* Q, int NQ, int kmax,
                                 float* cand_s, int* cand_i, hipStream_t st,
                                 const float* thr_init, int xcd, const int* gate) {
  if (NQ <= 0 || n_rblk <= 0) return 0;
  if (stride < 1 || n_valid < 0 || (kmax != 16 && kmax != 32)) return -1;
  if (!tiles || !n_live || !mask || (GROUPED && !qgroup)) return -1;
  const int n_qblk = (NQ + 255) / 256;
  const int aux = n_qblk == 1 ? 2 : 0;   // non-temporal when each index row is read by one block
#define SYMB_ARGS kmax, aux, X, n_valid, tiles, n_live, mask, qgroup, stride, n_rblk, Q, NQ, n_qblk, xcd, thr_init, cand_s, cand_i, st, gate
  switch (D) {
    case 256: return filter_fp8_dispatch<GROUPED, 256>(SYMB_ARGS);
    case 384: return filter_fp8_dispatch<GROUPED, 384>(SYMB_ARGS);
    case 512: return filter_fp8_dispatch<GROUPED, 512>(SYMB_ARGS);
    case 768: return filter_fp8_dispatch<GROUPED, 768>(SYMB_ARGS);
    case 1024: return filter_fp8_dispatch<GROUPED, 1024>(SYMB_ARGS);
  }
#undef SYMB_ARGS
  return -1;
}

}  // namespace symb
