// The emitting e4m3 scan under ONE row mask: index_scan_emit_fp8_kernel (fp8_emit.h) at
// GROUPED = false, its entry point, and the gated zeroing of the candidate counters that both
// mask forms call.
#include "fp8_emit.h"

namespace symb {

// cand_n[0 .. NQ) = 0 under the scan's gate: with *gate == 0 the counters keep what they held
__global__ void emit_fp8_zero_kernel(int* __restrict__ cand_n, int NQ,
                                     const int* __restrict__ gate) {
  if (*gate == 0) return;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < NQ) cand_n[i] = 0;
}

int emit_fp8_zero_counts(int* cand_n, int NQ, const int* gate, hipStream_t st) {
  if (gate == nullptr) return (int)hipMemsetAsync(cand_n, 0, sizeof(int) * (size_t)NQ, st);
  hipLaunchKernelGGL(emit_fp8_zero_kernel, dim3((NQ + 255) / 256), dim3(256), 0, st, cand_n, NQ,
                     gate);
  return 0;
}

}  // namespace symb

using namespace symb;

// X / Q / tiles / n_live / mask: as symb_index_scan_filter_fp8.  thr[NQ] (required), cand_s /
// cand_i [NQ][cap], cand_n[NQ]: as symb_index_scan_mq_filter, in raw units (S^2 * cosine).
// zero_cnt = 0 appends to cand_n instead of zeroing it (fp8_emit.h).
int symb_index_scan_emit_fp8(const void* X, int n_valid, int D, const int* tiles,
                             const int* n_live, const void* mask, int n_rblk, const void* Q,
                             int NQ, const float* thr, float* cand_s, int* cand_i, int* cand_n,
                             int cap, hipStream_t st, int xcd, const int* gate, int zero_cnt) {
  return index_scan_emit_fp8<false>(X, n_valid, D, tiles, n_live, mask, nullptr, n_rblk, Q, NQ,
                                    thr, cand_s, cand_i, cand_n, cap, st, xcd, gate, zero_cnt);
}
