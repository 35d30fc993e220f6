// The emitting e4m3 scan under a row mask, one kernel for both mask forms:
// index_scan_filter_fp8_kernel (fp8_filter_scan.h) with its per-lane register top-k replaced by
// the threshold emission of index_scan_mq_filter_kernel (index_mq_filter.hip).  It serves fp8
// shards at 32 < k <= 128, masked, tombstoned or (under an all-ones mask) plain, where no register
// list fits: every ALLOWED row scoring above the query's threshold (a lower bound on its final
// k-th allowed score) is appended to the query's candidate buffer, and the radix select takes the
// top k.  index_emit_fp8.hip instantiates GROUPED = false (one mask for every query),
// index_emit_group_fp8.hip GROUPED = true (a mask per query, up to MASK_GROUPS = 8 filters in a
// 256-query block: a query only ever emits rows of its own mask).
//
// From the list scan: 4 waves, 64 queries per wave as two 32-query B-fragment sets resident in
// AGPRs, v_mfma_f32_32x32x64_f8f6f4 through Fp8Chain (the same chain, so a row scores bit for bit
// what the list scan gives it: the search's threshold is a list-scan score and carries no
// margin), the Fp8Swz LDS image, the LDS-DMA ring with counted vmcnt and a raw barrier at
// Fp8Cfg<D>'s depth, the workgroup's slice of the live-tile list with n_live read on the device,
// tile_ptr / half_row clamping every list read to the slice's last interval, the batch of NS
// scalar loads in the prologue and the scalar state one interval ahead, live_word, mask_rows.
// Without the register lists four fragment reads are in flight at every width (the list scan
// keeps three at 1024).  No stride: the seed passes of the search stay the list scan.
//
// From index_scan_mq_filter_kernel: the fixed per-query threshold thr[NQ] (raw units, S^2 *
// cosine), the per-wave LDS stage of (raw score, physical row, query-in-wave) behind the ring
// (mq::STW entries, flushed before a 64-lane ballot could overflow it), the flush that takes
// slot = atomicAdd(cand_n + q, 1) and stores only below cap.  Queries at or past NQ (clamped for
// loading) hold thr = +inf and never emit, their counters do not exist.
//
// What GROUPED changes is where the mask words come from and how they are applied; every such
// site is an `if constexpr` below.
//  - single mask: `mask` is uint64 [n_words], qgroup is null.  The tile's word comes by one
//    s_load_dwordx2 and stays in SGPRs (w0; w1 is unused); mask_rows clears both query sets
//    under the same wave-uniform bits, and a sub-tile whose 32 bits are 0 is skipped by a
//    wave-uniform return.
//  - grouped (mask_group.h): `mask` is uint64 [n_words][8], qgroup int32 [NQ], & 7, clamped like
//    the fragments; tiles / n_live = filter_tiles of the OR of the slots.  As in the grouped list
//    scan a lane carries its two queries' group ids in one VGPR and two picked words w0 / w1;
//    the s_load_dwordx16 of the NEXT tile's words is issued at the barrier and waited for at the
//    interval's end with the tile indices (the list scan's placement below kmax 32: there are no
//    register lists here, so no update fills the SGPR file), pick2 cuts the two picked words at
//    n_valid, mask_rows takes a select per set and the wave-vote all-ones shortcut.
//  - grouped, the zero-bits skip: the bits are per lane while the emission holds ballots and a
//    wave-uniform stage count, so the skip is a wave VOTE -- no lane has a bit in b0 | b1 -- and
//    never a per-lane exit.  A tile of the union may be dead for every query of one wave and
//    live for another wave's; a lane whose own bits are 0 inside a live sub-tile holds -inf in
//    all sixteen accumulators of that set, and the test is the strict >, so even thr = -inf
//    emits nothing for it.
//
// Register budget: profiles/fold_masked_scans/README.md.
#pragma once
#include "fp8_scan.h"
#include "mask_group.h"
#include "mq_scan.h"

namespace symb {

// max of a lane's 16 accumulators by v_max3 (fmaxf would add NaN-canonicalising maxes)
__device__ __forceinline__ float fp8_max16(const f32x16& a) {
  float m;
  asm volatile(
      "v_max3_f32 %0, %1, %2, %3\n\t"
      "v_max3_f32 %0, %0, %4, %5\n\t"
      "v_max3_f32 %0, %0, %6, %7\n\t"
      "v_max3_f32 %0, %0, %8, %9\n\t"
      "v_max3_f32 %0, %0, %10, %11\n\t"
      "v_max3_f32 %0, %0, %12, %13\n\t"
      "v_max3_f32 %0, %0, %14, %15\n\t"
      "v_max3_f32 %0, %0, %16, %16"
      : "=&v"(m)
      : "v"(a[0]), "v"(a[1]), "v"(a[2]), "v"(a[3]), "v"(a[4]), "v"(a[5]), "v"(a[6]), "v"(a[7]),
        "v"(a[8]), "v"(a[9]), "v"(a[10]), "v"(a[11]), "v"(a[12]), "v"(a[13]), "v"(a[14]),
        "v"(a[15]));
  return m;
}

// cand_n[0 .. NQ) = 0 on stream st, under the scan's gate when there is one: with *gate == 0
// the counters keep what they held.  The kernel behind it is defined once, in
// index_emit_fp8.hip (each .hip is its own translation unit; both scans call this).
int emit_fp8_zero_counts(int* cand_n, int NQ, const int* gate, hipStream_t st);

// X: [>= round_up(n_valid, 64), D] e4m3 rows (scale S); Q: [NQ, D] e4m3 queries (scale S).
// tiles / n_live_p: filter_tiles' output for `mask` (GROUPED: the OR of its slots) at this
// n_valid; mask: the words it read.  qgroup: [NQ] group ids when GROUPED, else null.
// thr[NQ] (required): per-query lower bounds on the final k-th ALLOWED score, raw units.
// cand_s / cand_i: [NQ][cap] raw scores / physical rows; cand_n[NQ]: candidates each query emitted
// (may exceed cap; nothing is written at or past cap, and the select kernel raises the overflow
// flag).  gate (optional): run only if *gate != 0.
template <int D, int NS, int SUBS, int AUX, bool GROUPED>
__global__ __launch_bounds__(256, 1) void index_scan_emit_fp8_kernel(
    const uint8_t* __restrict__ X, int n_valid, const int* __restrict__ tiles,
    const int* __restrict__ n_live_p, const uint64_t* __restrict__ mask,
    const int* __restrict__ qgroup, const uint8_t* __restrict__ Q, int NQ, int n_qblk, int xcd,
    const float* __restrict__ thr_in, float* __restrict__ cand_s, int* __restrict__ cand_i,
    int* __restrict__ cand_n, int cap, const int* __restrict__ gate) {
  if (gate != nullptr && *gate == 0) return;   // (grid-uniform, before any barrier)
  constexpr int CPR = D / 16, SUB = 32, TR = 32 * SUBS, NW = 4;
  constexpr int IPE = 64 / TR;                     // barrier intervals per list entry
  constexpr int TILE_BYTES = TR * D, SUB_BYTES = SUB * D;
  constexpr int LOADS = TILE_BYTES / (1024 * NW);  // DMA pieces per wave per interval
  constexpr int NKS = D / 64, PF = 4, R = PF + 1;  // fragment reads in flight
  constexpr int STW = mq::STW, STAGE_BYTES = mq::STAGE_BYTES;
  static_assert((D % 256 == 0 || D == 384) && TILE_BYTES % (1024 * NW) == 0, "fp8 scan geometry");
  static_assert(SUBS == 1 || SUBS == 2, "an interval is half a list entry or a whole one");
  using Swz = Fp8Swz<D>;
  constexpr int G = Swz::G;
  static_assert(NS >= 2 && NS * TILE_BYTES + NW * STAGE_BYTES <= 160 * 1024,
                "LDS ring + stages exceed the CU's 160 KiB");
  static_assert(LOADS <= NKS, "DMA pieces must fit the first chain");
  static_assert(LOADS * (NS - 2) < 64, "vmcnt range");
  static_assert(STW >= 128 && STAGE_BYTES >= STW * 10, "stage: a 64-lane ballot past STW - 64");

  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wave_u = __builtin_amdgcn_readfirstlane(wave);
  const int lb = xcd ? xcd_remap(blockIdx.x, gridDim.x) : blockIdx.x;
  const int qb = lb % n_qblk, rb = lb / n_qblk;
  const int n_rblk = gridDim.x / n_qblk;
  const int h = lane >> 5;

  // ---- this workgroup's slice of the live-tile list ----
  const int n_live = __builtin_amdgcn_readfirstlane(*n_live_p);
  const int per = (n_live + n_rblk - 1) / n_rblk;
  const int slice_begin = __builtin_amdgcn_readfirstlane(min(rb * per, n_live));
  const int slice_len = max(min(per, n_live - slice_begin), 0);          // entries walked
  const int n_iv = __builtin_amdgcn_readfirstlane(slice_len * IPE);      // barrier intervals
  // interval iv (clamped to the last one) -> its entry's position in the list / its first row
  // within that entry's tile.  Called with n_iv > 0 only.  (readfirstlane: the scalar loads take
  // an SGPR address, and the compiler may select the clamp of a constant iv on the vector ALU)
  auto tile_ptr = [&](int iv) {
    return tiles + slice_begin + __builtin_amdgcn_readfirstlane(min(iv, n_iv - 1) / IPE);
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
  // padding queries never emit: their counters do not exist
  const float thr0 = query0 < NQ ? thr_in[query0] : INFINITY;
  const float thr1 = query1 < NQ ? thr_in[query1] : INFINITY;
  // grouped: the lane's two mask groups in one register, set 0's in bits 0-2 and set 1's in
  // bits 4-6 (padded lanes take the last query's, like its fragments).  The threshold (and
  // group) loads are consumed before any LDS-DMA is in flight (index_mq.hip)
  int grps = 0;
  if constexpr (GROUPED) {
    grps = (qgroup[min(query0, NQ - 1)] & (MASK_GROUPS - 1)) |
           ((qgroup[min(query1, NQ - 1)] & (MASK_GROUPS - 1)) << 4);
    asm volatile("" ::"v"(thr0), "v"(thr1), "v"(grps));
  } else {
    asm volatile("" ::"v"(thr0), "v"(thr1));
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

  // grouped: the lane's two words out of a tile's eight, cut at n_valid
  auto pick2 = [&](const u32x16& w8, int tile, uint64_t& w0, uint64_t& w1) {
    const uint64_t cut = live_word(~0ull, tile, n_valid);
    // (opaque: the fourteen compares against the group ids are loop invariants, and hoisted
    // out of the interval loop their masks are 28 SGPRs held across it)
    // (pick_word's plain form: the sequenced one changes no register figure here, the SGPR
    // file is not full without the register lists)
    int g = grps;
    asm volatile("" : "+v"(g));
    w0 = pick_word(w8, g & 15) & cut;
    w1 = pick_word(w8, g >> 4) & cut;
  };
  // row of accumulator register r within the 32-row sub-tile = 4 h + acc_reg_row(r), for both
  // query sets; b0 / b1: the sub-tile's 32 mask bits of the lane's set 0 / set 1 query, bit j =
  // row j allowed.  Single mask: b0 is wave-uniform and serves both sets.  Grouped: the
  // shortcut is a wave vote over both sets (fp8_filter_scan.h).
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

  // ---- candidate emission (the stage and its flush: index_scan_mq_kernel) --------------------
  char* stage = smem + NS * TILE_BYTES + wave_u * STAGE_BYTES;
  float* st_s = reinterpret_cast<float*>(stage);
  int* st_r = reinterpret_cast<int*>(stage + STW * 4);
  uint16_t* st_q = reinterpret_cast<uint16_t*>(stage + STW * 8);
  int nst = 0;  // staged entries (wave-uniform)
  auto flush = [&]() {
    int qw = qb * 256 + wave_u * 64;
    asm volatile("" : "+v"(qw));
    for (int e = lane; e < nst; e += 64) {
      const int q = qw + st_q[e];
      const int slot = atomicAdd(cand_n + q, 1);
      if (slot < cap) {
        cand_s[(size_t)q * cap + slot] = st_s[e];
        cand_i[(size_t)q * cap + slot] = st_r[e];
      }
    }
    nst = 0;
  };
  // the cold path of one query set: lane holds rows lrow + acc_reg_row(r) for query-in-wave lq
  auto emit_set = [&](const f32x16& acc, float mx, float thr, int lrow, int lq) {
    if (!__builtin_amdgcn_ballot_w64(mx > thr)) return;   // usually one set hits
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const bool p = acc[r] > thr;
      const uint64_t m = __builtin_amdgcn_ballot_w64(p);
      if (m) {
        if (nst > STW - 64) flush();
        const int idx = nst + (int)__builtin_amdgcn_mbcnt_hi(
                                  (uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0));
        if (p) {
          st_s[idx] = acc[r];
          st_r[idx] = lrow + acc_reg_row<true>(r);
          st_q[idx] = (uint16_t)lq;
        }
        nst += __builtin_popcountll(m);
      }
    }
  };
  // one 32-row sub-tile at physical row prow0; b0 / b1: its 32 mask bits as for mask_rows.
  // Every branch here is wave-uniform: emit_set holds ballots and the wave-uniform nst.
  auto emit = [&](f32x16& a0, f32x16& a1, int prow0, uint32_t b0, uint32_t b1) {
    // no allowed row (grouped: for any query of this wave, a vote, header note): nothing to
    // test (the chain ran all the same)
    if constexpr (!GROUPED) {
      if (b0 == 0u) return;
    } else {
      if (!__builtin_amdgcn_ballot_w64((b0 | b1) != 0u)) return;
    }
    mask_rows(a0, a1, b0, b1);
    const float mx0 = fp8_max16(a0), mx1 = fp8_max16(a1);
    if (__builtin_amdgcn_ballot_w64(mx0 > thr0 || mx1 > thr1)) {
      // cold path: per-lane values come from an opaque copy made here, so nothing it derives can
      // be hoisted out of the loop into the register budget
      int lo = lane;
      asm volatile("" : "+v"(lo));
      const int lrow = prow0 + 4 * (lo >> 5), lq = lo & 31;
      emit_set(a0, mx0, thr0, lrow, lq);
      emit_set(a1, mx1, thr1, lrow, lq + 32);
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
    // next interval's scalar state (waited for at the end of this interval)
    int n_nxt, n_pf;
    uint64_t n_w;
    u32x16 n_w8;
    sload_i32(n_nxt, tile_ptr(t + 2));
    sload_i32(n_pf, tile_ptr(t + NS));
    if constexpr (GROUPED)
      sload_mask8(n_w8, mask + (size_t)MASK_GROUPS * t_nxt);
    else
      sload_u64(n_w, mask + t_nxt);

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
      if (sub == 0) {
        fp8_prologue<0, PF, R, G>(lo, hi, voff, base);
        Fp8Chain<0, NKS, PF, LOADS, G>::run(acc0, acc1, lo, hi, q0, q1, voff, base, dma);
      } else {
        Fp8Chain<0, NKS, PF, 0, G>::run(acc0, acc1, lo, hi, q0, q1, voff, base, NoDma());
      }
      if (sub + 1 < SUBS)  // next sub-tile's first fragments fly during this test
        fp8_prologue<0, PF, R, G>(lo, hi, voff, base + SUB_BYTES);
      // (reads of the asm MFMA results stay below the chain-end s_nops: index_i8.hip emit)
      asm volatile("" : "+v"(acc0), "+v"(acc1));
      emit(acc0, acc1, row0 + sub * SUB, (uint32_t)(w0 >> (h0 + sub * SUB)),
           (uint32_t)(w1 >> (h0 + sub * SUB)));
    }

    if constexpr (GROUPED) {
      swait_mask8(n_nxt, n_pf, n_w8);
      pick2(n_w8, t_nxt, w0, w1);
    } else {
      swait(n_nxt, n_pf, n_w);
    }
    t_cur = t_nxt;
    t_nxt = n_nxt;
    t_pf = n_pf;
    if constexpr (!GROUPED) w0 = live_word(n_w, t_cur, n_valid);
  }
  if (nst) flush();
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // tail prefetches and emissions
}

template <bool GROUPED, int D, int AUX>
static int launch_emit_fp8(const void* X, int n_valid, const int* tiles, const int* n_live,
                           const void* mask, const int* qgroup, int n_rblk, const void* Q, int NQ,
                           int n_qblk, int xcd, const float* thr, float* cs, int* ci, int* cn,
                           int cap, hipStream_t st, const int* gate) {
  constexpr int SUBS = Fp8Cfg<D>::SUBS, NS = Fp8Cfg<D>::NS;
  constexpr int lds = NS * 32 * SUBS * D + 4 * mq::STAGE_BYTES;
  set_max_lds<index_scan_emit_fp8_kernel<D, NS, SUBS, AUX, GROUPED>>(lds);
  hipLaunchKernelGGL((index_scan_emit_fp8_kernel<D, NS, SUBS, AUX, GROUPED>),
                     dim3(n_rblk * n_qblk), dim3(256), lds, st, (const uint8_t*)X, n_valid, tiles,
                     n_live, (const uint64_t*)mask, qgroup, (const uint8_t*)Q, NQ, n_qblk, xcd,
                     thr, cs, ci, cn, cap, gate);
  return (int)hipGetLastError();
}

// The body of both entry points: argument checks, the counters' zeroing, then the width switch.
// qgroup is required when GROUPED and ignored (pass null) otherwise.  The grid is n_rblk row
// slots x ceil(NQ / 256) query blocks, the slots sharing the live tiles evenly.  zero_cnt = 0
// appends to cand_n instead of zeroing it; with a gate the zeroing is gated too, so a closed gate
// leaves every buffer as it was.
template <bool GROUPED>
static int index_scan_emit_fp8(const void* X, int n_valid, int D, const int* tiles,
                               const int* n_live, const void* mask, const int* qgroup, int n_rblk,
                               const void* Q, int NQ, const float* thr, float* cand_s, int* cand_i,
                               int* cand_n, int cap, hipStream_t st, int xcd, const int* gate,
                               int zero_cnt) {
  if (NQ <= 0) return 0;
  if (n_rblk <= 0 || n_valid < 0 || thr == nullptr || cap <= 0) return -1;
  if (!X || !Q || !tiles || !n_live || !mask || (GROUPED && !qgroup) || !cand_s || !cand_i ||
      !cand_n)
    return -1;
  if (D != 256 && D != 384 && D != 512 && D != 768 && D != 1024) return -1;
  if (zero_cnt) {
    const int e = emit_fp8_zero_counts(cand_n, NQ, gate, st);
    if (e) return e;
  }
  const int n_qblk = (NQ + 255) / 256;
  const int aux = n_qblk == 1 ? 2 : 0;   // non-temporal when each index row is read by one block
#define SYMB_E(D_) (aux ? launch_emit_fp8<GROUPED, D_, 2>(X, n_valid, tiles, n_live, mask, qgroup, n_rblk, Q, NQ, n_qblk, xcd, thr, cand_s, cand_i, cand_n, cap, st, gate) \
                        : launch_emit_fp8<GROUPED, D_, 0>(X, n_valid, tiles, n_live, mask, qgroup, n_rblk, Q, NQ, n_qblk, xcd, thr, cand_s, cand_i, cand_n, cap, st, gate))
  switch (D) {
    case 256: return SYMB_E(256);
    case 384: return SYMB_E(384);
    case 512: return SYMB_E(512);
    case 768: return SYMB_E(768);
    case 1024: return SYMB_E(1024);
  }
#undef SYMB_E
  return -1;
}

}  // namespace symb
