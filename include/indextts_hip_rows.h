/*
 * indextts_hip_rows.h -- entry points of libindextts_hip.so that take their per-row settings from a device table.
 *
 * Part of the C ABI (ITTS_ABI_VERSION 9, no struct of indextts_hip.h changed); indextts_hip.h includes it, it is not meant to be
 * included alone.  indextts_hip.h declares the base set of entry points, which the test suite enumerates one by one
 * (_native.EXPORTED_SYMBOLS, tests/test_native_abi.py, tests/test_host_launch_cpu.py); this header declares the entry points that
 * read their settings row by row from device memory (_native.ROW_SYMBOLS).  The same rule holds for it and is checked by
 * tests/test_row_sampling_cpu.py: every prototype below is exported by the library and bound by the Python side.
 * The record itts_sample_row and its layout are documented in indextts_hip.h, next to itts_sample.
 */
#ifndef INDEXTTS_HIP_ROWS_H
#define INDEXTTS_HIP_ROWS_H

typedef struct itts_sample_rows_args {
  const float* logits;
  int B, V, ldl;
  int32_t* tokens;
  int32_t* history;
  int hist_cap;
  int32_t* finished;
  int32_t* state;
  const int32_t* extra_ids;
  int n_extra;
  const int32_t* force_stop;
  const itts_sample_row* rows; /* [B] on the device */
  int stop_token;
  float* dbg_scores;
  int no_advance;
  const int32_t* row_step0;
} itts_sample_rows_args;
int itts_sample_rows(const itts_sample_rows_args* a, void* stream);

#endif
