/*
 * indextts_hip_prompts.h -- the prompt front-end over N prompts of different lengths in one launch each.
 *
 * Part of the C ABI (ITTS_ABI_VERSION 9, no struct of indextts_hip.h changed); indextts_hip.h includes it, it is not meant to be
 * included alone.  The Python side lists these entry points as _native.PROMPT_SYMBOLS (tests/test_prompt_batch_cpu.py holds the
 * list against this header).
 *
 * The row-wise launches of the conditioner (the GEMMs, itts_rows, itts_geglu) run unchanged over the concatenated rows of all
 * prompts.  The three launches that mix rows of a sequence -- the subsampling convolution, the attention and the convolution
 * module -- exist here in a segmented form: the same kernel bodies as itts_subsample_conv, itts_mha_small and
 * itts_glu_dwconv_ln_silu behind a segment lookup, and a segment's result has the bits the single-prompt entry point gives for
 * that segment alone.
 *
 * Row space.  Segment s owns rows [row0, row0 + len) of the launch's row space, row0 a multiple of 16: a 16-row tile of a packed
 * operand never holds rows of two segments.  The rows between a segment's end and the next multiple of 16 are padding rows:
 * row-wise launches may compute on them, no entry point here reads them as data or writes them.
 *
 * Segment table.  int32 words: nseg records of ITTS_SEG_WORDS words, then `ntiles` words that name the segment of every 16-row
 * tile of the row space (-1: none).  It exists twice: `dev` in device memory is what the kernels read -- device DATA, so a captured
 * graph depends on the geometry (nseg, ntiles, and through the caller's buffers the lengths), never on the pointer's contents
 * being known at capture time -- and `host`, the same words in host memory, which the entry point checks (row0 % 16, len > 0,
 * no tile in two segments, every range inside its buffer) before it launches: an invalid table returns ITTS_ERR_INVALID and
 * launches nothing.  The caller keeps the two copies equal.
 *
 *   word  itts_subsample_conv_seg        itts_mha_small_seg                       itts_glu_dwconv_ln_silu_seg
 *   0     row0: first output row         row0: first query row                    row0: first row of x and y
 *   1     len = (T_p - 3) / 2 + 1        len: queries                             len: rows
 *   2     first frame of the prompt      first row of the first key range         -
 *   3     T_p: frames of the prompt      rows of the first key range (> 0)        -
 *   4     -                              first row of the second key range        -
 *   5     -                              rows of the second key range (0: none)   -
 *   6     -                              first output row (a multiple of 16)      -
 *   7     reserved (0)
 */
#ifndef INDEXTTS_HIP_PROMPTS_H
#define INDEXTTS_HIP_PROMPTS_H

#define ITTS_SEG_WORDS 8

typedef struct itts_seg_table {
  const int32_t* dev;  /* device: nseg * ITTS_SEG_WORDS + ntiles words */
  const int32_t* host; /* the same words in host memory */
  int nseg, ntiles;
} itts_seg_table;

/* itts_subsample_conv over N prompts: mel fp32 [frames][F] holds the prompts' frames one after another (segment s: frames
 * [word 2, word 2 + word 3)), a 3 x 3 stride-2 window never leaves its prompt; y T [ntiles * 16][C * F2], row row0 + t of a
 * segment = what itts_subsample_conv writes to row t for that prompt alone.  Rows of y outside every segment are not written. */
int itts_subsample_conv_seg(const float* mel, const float* w, const float* b, void* y, const itts_seg_table* tab, int frames, int F,
                            int C, int dtype, void* stream);

/* itts_mha_small over N segments, one (segment, head, 16-query tile) per workgroup.  The fields of `a` keep their meaning with
 * these differences: q / k / v point at row 0 of their row spaces, a->Tq = rows of q and a->Tk = rows of k and v that exist
 * (bounds of the table); a segment's queries are rows [row0, row0 + len) of q, its keys and values the rows of its first key
 * range followed by those of its second; pos is T [H][pos_tk][64] and, like bias_u / bias_v, indexed by the key's index WITHIN
 * its segment (pos_tk >= the longest segment's key count; the first Tk rows of every head are those of the single-prompt table
 * for Tk keys); the output of query i of a segment goes to row (word 6) + i of the packed out operand of a->out_mtp row tiles.
 * Output rows outside every segment are not written; the caller keeps the segments' output rows apart. */
int itts_mha_small_seg(const itts_mha_args* a, const itts_seg_table* tab, int pos_tk, void* stream);

/* itts_glu_dwconv_ln_silu over N segments of x T [ntiles * 16][2 C] -> packed y of y_mtp >= ntiles row tiles: the depthwise
 * taps see zeros beyond the segment's first and last row, never the neighbouring segment's rows.  Rows outside every segment
 * are neither read nor written. */
int itts_glu_dwconv_ln_silu_seg(const void* x, const float* w, const float* b, const float* ln_w, const float* ln_b, void* y,
                                const itts_seg_table* tab, int C, int taps, int y_mtp, float eps, int dtype, void* stream);

#endif
