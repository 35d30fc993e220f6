// The emitting bf16 scan under a row mask: index_scan_mq_kernel (index_mq.hip) made to walk the
// live-tile list the way index_scan_filter_kernel (index_filter.hip) does.  It serves the masked
// and tombstoned searches at 32 < k <= 128, where no per-lane register list fits: every ALLOWED
// row scoring above the query's threshold (a lower bound on its final k-th allowed score) is
// appended to the query's candidate buffer, and the radix select takes the top k.
//
// From index_scan_mq_kernel, unchanged: 8 waves, queries resident as B operands of the
// hand-issued v_mfma_f32_16x16x32_bf16, MqGeo<D> tiles and ring depth, the LDS-DMA ring with
// counted vmcnt and a raw barrier, the MqChain fragment pipeline, the per-wave LDS candidate stage
// with ballot-prefix slots, the late waves' half-phase offset (mq_scan.h, index_mq.hip).
//
// From index_scan_filter_kernel:
//  * workgroup rb walks the slice [rb * per, min((rb + 1) * per, n_live)) of the live-tile list,
//    per = ceil(n_live / n_rblk), n_live read on the device (the host sizes the grid as if every
//    tile were live and reads nothing back);
//  * a list entry is a 64-row tile = 64 / TR barrier intervals (1 at D = 384, 2 at 768, 4 at
//    1024); the DMA source of a ring slot is X + (tile * 64 + interval_in_entry * TR) * D;
//  * tile indices and mask words are wave-uniform: hand-issued scalar loads right after the
//    barrier, waited for at the END of the interval, one interval ahead of their use (the header
//    of index_filter.hip has the reason).  Every list read is clamped to the slice's last walked
//    interval, so a slice shorter than the ring re-loads its last interval and the counted vmcnt
//    stays exact;
//  * before the v_max3 test every accumulator whose row bit is clear goes to -inf.  live_word
//    clears the bits at or past n_valid, which replaces the unmasked kernel's row_end masking.
// Emitted row numbers are physical rows.  No tshift and no MqList: the list replaces both.
#include "mq_scan.h"

namespace symb {

// X: [>= round_up(n_valid, 64), D] bf16 unit rows; Q: [NQ, D] bf16 unit queries.
// tiles / n_live_p: filter_tiles' output for `mask` at this n_valid; mask: the words it read.
// thr[NQ] (required): per-query lower bounds on the final k-th ALLOWED score.
// cand_s / cand_i: [NQ][cap]; cand_n[NQ]: candidates each query emitted (may exceed cap; nothing
// is written at or past cap, and the select kernel raises the overflow flag).
// gate (optional): run only if *gate != 0.
template <int D, int NSET, int RSPLIT>
__global__ __launch_bounds__(512, 1) void index_scan_mq_filter_kernel(
    const __bf16* __restrict__ X, int n_valid, const int* __restrict__ tiles,
    const int* __restrict__ n_live_p, const uint64_t* __restrict__ mask,
    const __bf16* __restrict__ Q, int NQ, int n_qblk, int xcd, const float* __restrict__ thr_in,
    float* __restrict__ cand_s, int* __restrict__ cand_i, int* __restrict__ cand_n, int cap,
    const int* __restrict__ gate) {
  if (gate != nullptr && *gate == 0) return;   // (grid-uniform, before any barrier)
  using namespace mq;
  using G = MqGeo<D>;
  constexpr int NKS = G::NKS, TR = G::TR, NSUB = G::NSUB, NS = G::NS;
  constexpr int TILE_BYTES = G::TILE_BYTES, LOADS = G::LOADS;
  constexpr int IPE = 64 / TR;                // barrier intervals per list entry
  constexpr int SETS = NSET, QW = SETS * 16, QWAVES = WAVES / RSPLIT, QPB = QWAVES * QW;
  constexpr int NSW = NSUB / RSPLIT;          // 16-row sub-tiles per wave per interval
  static_assert(RSPLIT == 1 || (RSPLIT == 2 && NSUB % 2 == 0), "row split");
  static_assert(SETS >= 1 && SETS <= G::MAX_SETS, "query registers");
  static_assert(IPE * TR == 64, "a list entry is whole intervals");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wave_u = __builtin_amdgcn_readfirstlane(wave);
  const int lb = xcd ? xcd_remap(blockIdx.x, gridDim.x) : blockIdx.x;
  const int qb = lb % n_qblk, rb = lb / n_qblk;
  const int n_rblk = gridDim.x / n_qblk;

  // ---- this workgroup's slice of the live-tile list ----
  const int n_live = __builtin_amdgcn_readfirstlane(*n_live_p);
  const int per = (n_live + n_rblk - 1) / n_rblk;
  const int slice_begin = __builtin_amdgcn_readfirstlane(min(rb * per, n_live));
  const int slice_len = max(min(per, n_live - slice_begin), 0);        // entries walked
  const int n_iv = __builtin_amdgcn_readfirstlane(slice_len * IPE);    // barrier intervals
  // interval iv (clamped to the last one) -> its entry in the list / its first row within that
  // entry's 64-row tile
  // (readfirstlane: the scalar loads take an SGPR address, and the compiler may select the
  // clamp of a constant iv on the vector ALU)
  auto tile_ptr = [&](int iv) {
    return tiles + slice_begin + __builtin_amdgcn_readfirstlane(min(iv, n_iv - 1) / IPE);
  };
  auto sub_row = [&](int iv) { return (min(iv, n_iv - 1) % IPE) * TR; };

  // ---- query fragments (B operand, 16x16x32: lane holds Q[col = lane&15][k = 8*(lane>>4)+j]) --
  const int qwave = wave % QWAVES;                 // this wave's query group
  const int j0 = (wave_u / QWAVES) * NSW;           // this wave's first sub-tile of an interval
  const int qbase = qb * QPB + qwave * QW + (lane & 15);
  bf16x8 qf[SETS][NKS];
  float thr[SETS];
#pragma unroll
  for (int s = 0; s < SETS; ++s) {
    const int q = qbase + s * 16;
    const __bf16* qp = Q + (size_t)min(q, NQ - 1) * D + (lane >> 4) * 8;
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) qf[s][ks] = *reinterpret_cast<const bf16x8*>(qp + ks * 32);
    thr[s] = q < NQ ? thr_in[q] : INFINITY;   // padding queries never emit
  }
  // consume the query/threshold loads before any LDS-DMA is in flight (index_mq.hip)
#pragma unroll
  for (int s = 0; s < SETS; ++s) {
    asm volatile("" ::"v"(thr[s]));
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) asm volatile("" ::"v"(qf[s][ks]));
  }

  // ---- LDS-DMA: wave w fills pieces p = i*WAVES + w (i < LOADS) of an interval's tile; the
  // per-lane offset is index_scan_mq_kernel's.  row_base: the interval's first physical row
  // (wave-uniform, from the list); slot: the interval number (ring position).
  const uint32_t loff = (uint32_t)((lane >> 2) * D * 2 + (((lane & 3) ^ ((lane >> 3) & 2)) * 16));
  auto issue_piece = [&](int row_base, int slot, int i) {
    const int p = i * WAVES + wave_u, j = p / NKS, ks = p % NKS;
    const char* base = reinterpret_cast<const char*>(X + (size_t)(row_base + j * SUB) * D + ks * 32);
    char* dst = smem + (slot % NS) * TILE_BYTES + p * PIECE;
    glds16_aux<0>(mq_uniform(base) + loff, dst);
  };

  // ---- per-lane A-fragment offset within a piece (lane holds X[row r][k 8g..8g+7] of the k-step)
  const uint32_t lds_smem = lds_addr(smem);
  const uint32_t foff = (uint32_t)((lane & 15) * 64 + (((lane >> 4) ^ ((lane >> 1) & 2)) * 16));

  // ---- candidate emission (the stage and its flush: index_scan_mq_kernel) --------------------
  char* stage = smem + NS * TILE_BYTES + wave_u * STAGE_BYTES;
  float* st_s = reinterpret_cast<float*>(stage);
  int* st_r = reinterpret_cast<int*>(stage + STW * 4);
  uint16_t* st_q = reinterpret_cast<uint16_t*>(stage + STW * 8);
  int nst = 0;  // staged entries (wave-uniform)
  auto flush = [&]() {
    int qw = qb * QPB + (wave_u % QWAVES) * QW;
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
  // one 16-row sub-tile at physical row prow0 whose 16 mask bits are ``bits`` (wave-uniform, bit
  // j = row prow0 + j allowed): lane holds rows 4*(lane>>4) + r of it for the 16 queries of each
  // set (column lane & 15)
  auto emit = [&](f32x4 (&acc)[SETS], int prow0, uint32_t bits) {
    if (bits == 0u) return;   // no allowed row: nothing to test (the chain ran all the same)
    // keep every read of the inline-asm MFMA results below the chain-end s_nops
#pragma unroll
    for (int s = 0; s < SETS; ++s) asm volatile("" : "+v"(acc[s]));
    if (bits != 0xffffu) {    // (wave-uniform) disallowed rows never pass a threshold
      int lo = lane;
      asm volatile("" : "+v"(lo));
      const uint32_t lbits = bits >> (4 * (lo >> 4));
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const bool off = !((lbits >> r) & 1u);
#pragma unroll
        for (int s = 0; s < SETS; ++s)
          if (off) acc[s][r] = -INFINITY;
      }
    }
    // max of each set's 4 scores by two v_max3 (fmaxf would add NaN-canonicalising maxes)
    float mx[SETS];
#pragma unroll
    for (int s = 0; s < SETS; ++s)
      asm volatile("v_max3_f32 %0, %1, %2, %3\n\tv_max3_f32 %0, %0, %4, %4"
                   : "=&v"(mx[s]) : "v"(acc[s][0]), "v"(acc[s][1]), "v"(acc[s][2]), "v"(acc[s][3]));
    bool hit = false;
#pragma unroll
    for (int s = 0; s < SETS; ++s) hit |= mx[s] > thr[s];
    if (__builtin_amdgcn_ballot_w64(hit)) {
      // cold path: per-lane values come from opaque copies made here, so nothing it derives can
      // be hoisted out of the loop into the (full) register budget
      int lo = lane;
      asm volatile("" : "+v"(lo));
      const int lrow = prow0 + 4 * (lo >> 4), lq = lo & 15;
#pragma unroll
      for (int s = 0; s < SETS; ++s) {
        if (!__builtin_amdgcn_ballot_w64(mx[s] > thr[s])) continue;   // usually one set hits
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const bool p = acc[s][r] > thr[s];
          const uint64_t m = __builtin_amdgcn_ballot_w64(p);
          if (m) {
            if (nst > STW - 64) flush();
            const int idx = nst + (int)__builtin_amdgcn_mbcnt_hi(
                                      (uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0));
            if (p) {
              st_s[idx] = acc[s][r];
              st_r[idx] = lrow + r;
              st_q[idx] = (uint16_t)(s * 16 + lq);
            }
            nst += __builtin_popcountll(m);
          }
        }
      }
    }
  };

  // Scalar state, one interval ahead: t_cur / w_cur = tile and live mask word of interval t,
  // t_nxt = tile of interval t + 1, t_pf = tile of the interval prefetched during t (t + NS - 1).
  int t_cur = 0, t_nxt = 0, t_pf = 0;
  uint64_t w_cur = 0;
  if (n_iv > 0) {
    // tiles of intervals 0 .. NS - 1 (at D = 1024 the first four are one entry; short slices
    // clamp): the ring's first NS - 1 slots, t_nxt and t_pf all come from them
    int tp[NS];
#pragma unroll
    for (int p = 0; p < NS; ++p) sload_i32(tp[p], tile_ptr(p));
    swait_n(tp);
    sload_u64(w_cur, mask + tp[0]);
#pragma unroll
    for (int p = 0; p < NS - 1; ++p)
#pragma unroll
      for (int i = 0; i < LOADS; ++i) issue_piece(tp[p] * 64 + sub_row(p), p, i);
    t_cur = tp[0];
    t_nxt = tp[1];
    t_pf = tp[NS - 1];
    swait(t_cur, t_nxt, w_cur);
    w_cur = live_word(w_cur, t_cur, n_valid);
  }
  bf16x8 a[R];
  f32x4 acc[SETS];
  // The late waves (index_mq.hip) test their last sub-tile of interval t - 1 AFTER the barrier
  // of interval t, so they carry that sub-tile's physical row and its 16 mask bits across the
  // barrier: by then t_cur / w_cur describe interval t, another tile or another part of the word.
  const bool late = wave_u >= WAVES / 2;
  const int last = (j0 + NSW - 1) * SUB;   // row offset of this wave's last sub-tile
  int prow_last = 0;
  uint32_t bits_last = 0;
  for (int t = 0; t < n_iv; ++t) {
    // interval t landed for this wave once only the (NS-2) younger intervals' pieces remain; the
    // barrier makes every wave's pieces visible and retires every wave's reads of slot (t-1) % NS
    wait_vmcnt<LOADS * (NS - 2)>();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    // next interval's scalar state (waited for at the end of this interval)
    int n_nxt, n_pf;
    uint64_t n_w;
    sload_i32(n_nxt, tile_ptr(t + 2));
    sload_i32(n_pf, tile_ptr(t + NS));
    sload_u64(n_w, mask + t_nxt);

    const uint32_t tbase = lds_smem + (uint32_t)((t % NS) * TILE_BYTES);
    const int h0 = sub_row(t);
    const int prow0 = t_cur * 64 + h0;
    const uint64_t wiv = w_cur >> h0;     // this interval's TR mask bits at the low end
    const int pf_row = t_pf * 64 + sub_row(t + NS - 1);
    const int tnext = t + NS - 1;
    auto dma = [&](int i) { issue_piece(pf_row, tnext, i); };
    auto sub_bits = [&](int off) { return (uint32_t)(wiv >> off) & 0xffffu; };
    const uint32_t fb = tbase + foff;   // this lane's fragment in piece 0 of sub-tile 0
    mq_prologue<0>(a, fb + j0 * NKS * PIECE);
    if (late && t > 0) emit(acc, prow_last + last, bits_last);
    prow_last = prow0;
    bits_last = sub_bits(last);
    const uint32_t fw = fb + j0 * NKS * PIECE;
    if constexpr (NSW > 1)
      MqChain<D, 0, LOADS, true, SETS>::run(acc, a, qf, fw, fw + NKS * PIECE, dma);
    else
      MqChain<D, 0, LOADS, false, SETS>::run(acc, a, qf, fw, 0, dma);
#pragma unroll
    for (int j = 1; j < NSW; ++j) {
      // sub-tile j's first fragments were read by the previous chain's tail and fly while this
      // wave tests the previous sub-tile's scores
      emit(acc, prow0 + (j0 + j - 1) * SUB, sub_bits((j0 + j - 1) * SUB));
      if (j + 1 < NSW)
        MqChain<D, 0, 0, true, SETS>::run(acc, a, qf, fw + j * NKS * PIECE,
                                          fw + (j + 1) * NKS * PIECE, NoDma());
      else
        MqChain<D, 0, 0, false, SETS>::run(acc, a, qf, fw + j * NKS * PIECE, 0, NoDma());
    }
    if (!late) emit(acc, prow0 + last, bits_last);

    swait(n_nxt, n_pf, n_w);
    t_cur = t_nxt;
    t_nxt = n_nxt;
    t_pf = n_pf;
    w_cur = live_word(n_w, t_cur, n_valid);
  }
  if (late && n_iv > 0) emit(acc, prow_last + last, bits_last);
  if (nst) flush();
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // tail prefetches and emissions
}

// cand_n[0 .. NQ) = 0 under the scan's gate: with *gate == 0 the counters keep what they held
__global__ void mq_filter_zero_kernel(int* __restrict__ cand_n, int NQ,
                                      const int* __restrict__ gate) {
  if (*gate == 0) return;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < NQ) cand_n[i] = 0;
}

}  // namespace symb

using namespace symb;

template <int D, int NSET, int RSPLIT>
static int launch_mq_filter(const void* X, int n_valid, const int* tiles, const int* n_live,
                            const void* mask, int n_rblk, const void* Q, int NQ, const float* thr,
                            float* cand_s, int* cand_i, int* cand_n, int cap, int xcd,
                            hipStream_t st, const int* gate) {
  constexpr int qpb = mq::WAVES / RSPLIT * 16 * NSET;
  const int n_qblk = (NQ + qpb - 1) / qpb;
  constexpr int lds = MqGeo<D>::LDS_BYTES;
  set_max_lds<index_scan_mq_filter_kernel<D, NSET, RSPLIT>>(lds);
  hipLaunchKernelGGL((index_scan_mq_filter_kernel<D, NSET, RSPLIT>), dim3(n_rblk * n_qblk),
                     dim3(512), lds, st, (const __bf16*)X, n_valid, tiles, n_live,
                     (const uint64_t*)mask, (const __bf16*)Q, NQ, n_qblk, xcd, thr, cand_s, cand_i,
                     cand_n, cap, gate);
  return (int)hipGetLastError();
}

// dim: 384 (sets 4; rsplit 1 or 2), 768 (sets 2, rsplit 1), 1024 (sets 1, rsplit 1).  Queries per
// workgroup: 8 / rsplit * 16 * sets (symb_mq_queries_per_blk).
// tiles / n_live: symb_filter_tiles' output for `mask` at this n_valid (every entry a tile below
// ceil(n_valid / 64)); the grid is n_rblk row slots x the query blocks, the slots sharing the
// live tiles evenly.  zero_cnt = 0 appends to cand_n instead of zeroing it; with a gate the
// zeroing is gated too, so a closed gate leaves every buffer as it was.
int symb_index_scan_mq_filter(const void* X, int n_valid, const int* tiles, const int* n_live,
                              const void* mask, int n_rblk, const void* Q, int NQ,
                              const float* thr, float* cand_s, int* cand_i, int* cand_n, int cap,
                              int xcd, hipStream_t st, int sets, int rsplit, const int* gate,
                              int zero_cnt, int dim) {
  if (NQ <= 0) return 0;
  if (n_rblk <= 0 || n_valid < 0 || thr == nullptr || cap <= 0) return -1;
  if (!tiles || !n_live || !mask || !cand_s || !cand_i || !cand_n) return -1;
  if (dim == 384 && (sets != 4 || (rsplit != 1 && rsplit != 2))) return -1;
  if (dim == 768 && (sets != 2 || rsplit != 1)) return -1;
  if (dim == 1024 && (sets != 1 || rsplit != 1)) return -1;
  if (dim != 384 && dim != 768 && dim != 1024) return -1;
  if (zero_cnt) {
    if (gate == nullptr) {
      hipError_t e = hipMemsetAsync(cand_n, 0, sizeof(int) * (size_t)NQ, st);
      if (e != hipSuccess) return (int)e;
    } else {
      hipLaunchKernelGGL(mq_filter_zero_kernel, dim3((NQ + 255) / 256), dim3(256), 0, st, cand_n,
                         NQ, gate);
    }
  }
#define SYMB_MQF(D_, S_, R_) launch_mq_filter<D_, S_, R_>(X, n_valid, tiles, n_live, mask, n_rblk, \
                                                         Q, NQ, thr, cand_s, cand_i, cand_n, cap, \
                                                         xcd, st, gate)
  if (dim == 768) return SYMB_MQF(768, 2, 1);
  if (dim == 1024) return SYMB_MQF(1024, 1, 1);
  return rsplit == 2 ? SYMB_MQF(384, 4, 2) : SYMB_MQF(384, 4, 1);
#undef SYMB_MQF
}
