/*
 * indextts_voice.h -- C ABI of libindextts_voice.so: the gfx950 (MI355X / CDNA4) kernel behind voice extraction
 * (indextts/gpt/voice_extract.py): products with the DIFFERENCE of two weight matrices, so that
 * the LoRA a merged fine-tuned checkpoint holds can be recovered without ever writing that difference to memory.
 *
 * A library of its own, beside libindextts_hip.so (include/indextts_hip.h), whose ABI it leaves alone: every name here
 * carries the prefix ittv_ / ITTV_.  Conventions as there: an entry point returns ITTV_OK (0) or an ITTV_ERR_* code, the
 * message is available from ittv_last_error() (thread-local); no exceptions cross the ABI, no hidden device allocations
 * (the workspace is passed in); the launch is asynchronous on `stream` (a hipStream_t passed as void*; NULL = default).
 */
#ifndef INDEXTTS_VOICE_H
#define INDEXTTS_VOICE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ITTV_OK 0
#define ITTV_ERR_INVALID 1 /* bad argument / unsupported shape (nothing was launched) */
#define ITTV_ERR_LAUNCH 2  /* HIP reported an error at launch */

#define ITTV_F32 0
#define ITTV_BF16 1
#define ITTV_F16 2

#define ITTV_ABI_VERSION 1

/* Bytes of workspace every ittv_delta_project call is given (the launch plan is a function of K, N, c and trans alone and
 * never needs more): 64 KiB of tile counters, then the fp32 slabs of a reduction split over several workgroups. */
#define ITTV_DELTA_WS_BYTES ((int64_t)(16 << 20) + (64 << 10))

int ittv_abi_version(void);
const char* ittv_last_error(void);

/* Y = op(D) X in one launch,  D[k][n] = float(wt[k][n]) - float(wb[k][n])  formed in registers (exact for two 16-bit
 * operands), products and sums in fp32.
 *   wt, wb   row-major [K][N] (the Conv1D layout of a checkpoint), of type dtype_t / dtype_b (ITTV_F32 / _BF16 / _F16,
 *            independently); every element is read once, with 16-byte loads
 *   trans 0  x fp32 [N][c] -> y fp32 [K][c] = D x          trans 1  x fp32 [K][c] -> y fp32 [N][c] = D^T x
 *   K, N     multiples of 16;  c a multiple of 16, 16 <= c <= 80;  all four pointers 16-byte aligned
 *   ws       ITTV_DELTA_WS_BYTES bytes of device memory (ws_bytes says how many there are), 16-byte aligned, used by this
 *            launch only: where the plan splits the reduction, every workgroup writes its partial tile there and the one that
 *            arrives last adds them IN SPLIT ORDER -- no floating-point atomics, the same inputs give the same bits.
 * The call enqueues one memset of the tile counters and one kernel. */
typedef struct ittv_delta_args {
  int dtype_t, dtype_b;
  int K, N, c, trans;
  const void* wt;
  const void* wb;
  const float* x;
  float* y;
  void* ws;
  int64_t ws_bytes;
} ittv_delta_args;

int ittv_delta_project(const ittv_delta_args* a, void* stream);

#ifdef __cplusplus
}
#endif
#endif
