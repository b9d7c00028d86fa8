/*
 * spmm_hip.h — C ABI of the MI355X-native SpMM engine (libspmm_hip.so).
 *
 * This is the drop-in boundary for the two hot paths of
 * xuyifangreeneyes/spmm-denseblock:
 *
 *   Path A  CSR x dense   replaces gespmm_csrmm<T>          (gespmm_csrmm.h:422-426)
 *                          and the legacy cusparseScsrmm / cusparseScsrmm2 call
 *                          sites (run_csrmm.cu:133-142, test_csrmm.cu:126-129)
 *   Path B  BSR x dense   replaces rocsparse_bsrmm_template<T> (rocsparse_bsrmm.h:102-256)
 *                          and cusparseSbsrmm (run_bsrmm.cu:160-165), plus the
 *                          per-block cublasSgemm variant (block_cublas.cu:123-136)
 *   Prep    csr2bsr / bsr2csr / nnzb on the HOST (north_star: conversion stays
 *           CPU-side preprocessing), replacing cusparseXcsr2bsrNnz +
 *           cusparseScsr2bsr (run_bsrmm.cu:116-142) and cusparseSbsr2csr
 *           (bsr2csr.cu:186-188).
 *
 * Conventions
 *   - Plain C: pointers, sizes, enums. No HIP or torch types in signatures;
 *     a stream is passed as an opaque `void*` (a hipStream_t, 0 = default).
 *   - The caller owns every device buffer (the reference cudaMallocs in its
 *     drivers). Kernels never allocate; a handle may keep a small internal
 *     workspace (merge-path carries, layout staging) that it grows lazily.
 *   - Numeric values of spmm_status_t / spmm_direction_t / spmm_operation_t
 *     mirror cusparseStatus_t / cusparseDirection_t / cusparseOperation_t so a
 *     caller's HANDLE_CUSPARSE_ERROR-style checks keep working.
 *   - All index arrays are int32, as in the reference. fp32 values unless the
 *     function name says otherwise.
 */
#ifndef SPMM_HIP_H
#define SPMM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SPMM_HIP_VERSION 100 /* 1.0.0 */

typedef enum {
  SPMM_STATUS_SUCCESS = 0,
  SPMM_STATUS_NOT_INITIALIZED = 1,
  SPMM_STATUS_ALLOC_FAILED = 2,
  SPMM_STATUS_INVALID_VALUE = 3,
  SPMM_STATUS_ARCH_MISMATCH = 4,
  SPMM_STATUS_MAPPING_ERROR = 5,
  SPMM_STATUS_EXECUTION_FAILED = 6,
  SPMM_STATUS_INTERNAL_ERROR = 7,
  SPMM_STATUS_MATRIX_TYPE_NOT_SUPPORTED = 8,
  SPMM_STATUS_ZERO_PIVOT = 9,
  SPMM_STATUS_NOT_SUPPORTED = 10
} spmm_status_t;

typedef enum { SPMM_DIRECTION_ROW = 0, SPMM_DIRECTION_COLUMN = 1 } spmm_direction_t;

typedef enum {
  SPMM_OPERATION_NON_TRANSPOSE = 0,
  SPMM_OPERATION_TRANSPOSE = 1,
  SPMM_OPERATION_CONJUGATE_TRANSPOSE = 2
} spmm_operation_t;

/* Storage order of a dense matrix (explicit in the *_ex entry points). */
typedef enum { SPMM_ORDER_ROW = 0, SPMM_ORDER_COL = 1 } spmm_order_t;

typedef enum { SPMM_INDEX_BASE_ZERO = 0, SPMM_INDEX_BASE_ONE = 1 } spmm_index_base_t;

typedef enum { SPMM_MATRIX_TYPE_GENERAL = 0 } spmm_matrix_type_t;

typedef struct spmm_context* spmm_handle_t;    /* ~ cusparseHandle_t  */
typedef struct spmm_mat_descr* spmm_mat_descr_t; /* ~ cusparseMatDescr_t */

/* ------------------------------------------------------------------------ */
/* Handle / descriptor lifecycle (cusparseCreate, cusparseSetStream, ...)     */
/* ------------------------------------------------------------------------ */
int spmm_get_version(void);
const char* spmm_get_status_string(spmm_status_t status);

spmm_status_t spmm_create(spmm_handle_t* handle);
spmm_status_t spmm_destroy(spmm_handle_t handle);
/* Streams. A handle's device buffers carry one call's state while its kernels
 * run (split-row tickets and partial sums, staged copies of B and C, segment
 * lists, probe sums), so the calls of one handle must run one after the other
 * on the device. On one stream they do. When the stream changes
 * (spmm_set_stream with another stream, or a handle-less spmm_gespmm_csrmm_*
 * entry called with a stream other than the default handle's current one), the
 * library keeps that order itself: the new stream is made to wait for
 * everything the handle has queued on the old one (an event recorded there)
 * before any buffer is looked at, grown or freed. Two streams fed through one
 * handle therefore never overlap; give streams that should run concurrently a
 * handle each (tests/test_gpu_stream_switch.py).
 *   Setting the stream the handle already has compares two pointers and queues
 *     nothing. A handle that owns no device buffer yet (a new one, or one
 *     whose calls so far have kept nothing in it) has nothing to order and
 *     just takes the stream.
 *   Capture: while the old or the new stream is being captured, a change that
 *     needs the order returns SPMM_STATUS_NOT_SUPPORTED before anything is
 *     recorded, waited for or synchronised; the handle keeps its old stream
 *     and the capture stays valid. Bind the handle to the capture stream
 *     before the capture begins.
 *   Lifetime: a stream must still exist when the handle next changes away
 *     from it (the event is recorded on it then). If it does not, the change
 *     waits for the whole device instead.
 *   Threads: one host thread at a time drives a handle, and the stream is
 *     part of that: it is read and written without a lock. This includes the
 *     process-wide default handle of the handle-less entries, whatever stream
 *     each caller passes. */
spmm_status_t spmm_set_stream(spmm_handle_t handle, void* stream);
spmm_status_t spmm_get_stream(spmm_handle_t handle, void** stream);

/* Graph capture. On a handle whose buffers are already large enough a product
 * queues kernels, memsets and device-to-device copies on the handle's stream
 * and nothing else, so it can be captured in a HIP graph (hipStreamBeginCapture
 * on that stream) and replayed: every replay re-reads rowptr / colind / val, B
 * and C at the captured addresses and returns the handle's tickets, flags and
 * sums to rest, and gives the bits of the eager call on those operands
 * (tests/test_gpu_graph_replay.py).
 *   Capturable, and tested so: spmm_csrmm_ex_f32 / _f16 / _f64 (any
 *     spmm_set_csr_waves_per_cu), spmm_csrmm_hot_f32, spmm_bsrmm_ex_f32 / _f16
 *     / _f64 (SPMM_BSR_SMALL_GROUPED included), spmm_hybrid_csrmm_f32 /
 *     _ex_f32, spmm_bsrmm_grouped_f16 / _f32, spmm_sddmm_csr_f32 and
 *     spmm_edge_softmax_csr_f32 / _bwd_csr_f32 and their multi-head forms
 *     spmm_sddmm_csr_heads_f32 / _f16 / _bf16, spmm_edge_softmax_csr_heads_f32 /
 *     _bwd_csr_heads_f32 and spmm_csrmm_heads_f32 / _f16 / _bf16 and the max /
 *     min reducers spmm_csrmm_reduce_f32 / _bwd_f32 (which keep
 *     nothing in the handle's buffers), and the filling call of a group
 *     analysis. The setters of handle options are host-only: what they set is
 *     baked into the launches captured after them.
 *   Not capturable (they hand a size or a flag back to the host, and
 *     synchronise for it): the analyses that return a size (the size query of
 *     a group analysis), the device converters (spmm_xcsr2bsr_nnz_dev,
 *     spmm_scsr2bsr_dev, spmm_sbsr2csr_dev, spmm_xbsr_reblock32_nnzb /
 *     spmm_sbsr_reblock32, spmm_csr2csc_dev), spmm_bsr_small_path and
 *     spmm_get_kernel_times. Run them before the capture. spmm_csr2csc_dev
 *     checks for a capture itself and returns SPMM_STATUS_NOT_SUPPORTED
 *     before it queues anything.
 *   Precondition: one eager call with the same arguments on the same handle
 *     beforehand (it sizes the handle's buffers), and kernel timing off. A
 *     call that would have to grow a buffer while the handle's stream is
 *     capturing returns SPMM_STATUS_NOT_SUPPORTED before it synchronises,
 *     frees or allocates anything; the capture itself stays valid. The
 *     handle is on the capture stream before the capture begins: setting
 *     that same stream again inside the capture adds nothing to the graph,
 *     while a change of stream on a handle that owns buffers is refused in
 *     the same way ("Streams" above).
 *   Lifetime: a graph holds pointers into the handle's buffers. The handle must
 *     outlive its graphs, and any later call on that handle that grows a buffer
 *     (a larger shape, another entry) frees what earlier graphs point to:
 *     capture again after it. The handle-less spmm_gespmm_csrmm_* entries use
 *     the process-wide default handle, so for them the rule spans every caller
 *     in the process. */

spmm_status_t spmm_create_mat_descr(spmm_mat_descr_t* descr);
spmm_status_t spmm_destroy_mat_descr(spmm_mat_descr_t descr);
spmm_status_t spmm_set_mat_type(spmm_mat_descr_t descr, spmm_matrix_type_t type);
spmm_status_t spmm_set_mat_index_base(spmm_mat_descr_t descr, spmm_index_base_t base);

/* Per-launch device timing of the dominant kernel (hipEvents recorded on the
 * handle's stream around each main-kernel launch). Used by bench.py for the
 * roofline figure; off by default, costs two event records per launch. */
spmm_status_t spmm_set_kernel_timing(spmm_handle_t handle, int enable);
/* Synchronises the recorded events, returns up to max_count durations (ms),
 * oldest first, and clears the record. */
spmm_status_t spmm_get_kernel_times(spmm_handle_t handle, float* ms, int max_count, int* count);

/* Launch record (a test aid: which kernel instantiations a call queued). While
 * on, every kernel launch made through the handle appends one identifier, in
 * launch order: the mangled name of a tag type that holds the kernel's own
 * symbol with its template arguments (csrc/kernel_tag.hpp; tests/kernel_keys.py
 * maps it onto the .amdhsa_kernel symbol). Host-side only: it records what was
 * queued, also while the stream is capturing, reads no device memory and does
 * not synchronise. Like every call on a handle it is for the one host thread
 * that drives the handle (the list is appended to without a lock; this holds
 * for the default handle of the handle-less entries too). Off by default,
 * where a launch costs one test of a flag;
 * enabling it clears the record, disabling it keeps what was recorded. */
spmm_status_t spmm_set_launch_record(spmm_handle_t handle, int enable);
/* Up to max_count identifiers, oldest first; *count = how many were written.
 * The strings are static: they stay valid for the life of the library. The
 * record is not cleared (spmm_set_launch_record(handle, 1) does that). */
spmm_status_t spmm_get_launch_record(spmm_handle_t handle, const char** ids, int max_count,
                                     int* count);

/* Tuning knob for the CSR merge-path kernel: resident waves per CU the grid
 * is sized for (0 = default). The edge softmax's kernel takes it too: that many
 * waves per CU share the rows, however few each then gets (its bits are the
 * row's at any grid). */
spmm_status_t spmm_set_csr_waves_per_cu(spmm_handle_t handle, int waves_per_cu);
/* The target a handle without that setting sizes a CSR launch's grid for: 16
 * waves per CU, 12 from 2^20 rows on the plain kernel (hot != 0: the
 * spmm_csrmm_hot_f32 kernel, which keeps 16). Host-only; the result of the
 * product does not depend on it. */
int spmm_csr_default_waves_per_cu(int m, int hot);

/* CSR kernel options (bit flags). SPMM_CSR_NT_STREAMS: read colind/val and
 * write C with non-temporal hints, keeping L2 / MALL for the B gathers. */
#define SPMM_CSR_NT_STREAMS 1
/* K <= 32: use the one-nnz-per-wave-instruction kernel (one sequential FMA
 * chain per unsplit row, the reference's order) instead of the default
 * several-rows-per-instruction kernel (interleaved chains per row). */
#define SPMM_CSR_SEQUENTIAL_ROWS 2
spmm_status_t spmm_set_csr_options(spmm_handle_t handle, int flags);

/* BSR kernel options (bit flags, per handle).
 *
 * The default contract of the BSR entries at bs 16 / 32 (the column streams,
 * DESIGN.md §4) is COLUMN-GRANULAR: a column of a stored block whose values
 * are all +-0 is skipped; every other column multiplies whole, its explicit
 * zeros included. With finite B this is the dense block product exactly. With
 * an inf / NaN in B row J*bs + c, rows of block row I get a non-finite value
 * from it iff a stored block (I, J) holds a value other than +-0 in its
 * column c: then every row of block row I does (0 * inf = NaN for the rows
 * whose entry is an explicit zero), and if column c is all zeros none does.
 *
 * SPMM_BSR_DENSE_BLOCK_PRODUCT: cusparseSbsrmm's dense-block semantics
 * (bsrmm.cu:141-144): every stored block multiplies as a dense
 * bs x bs matrix, so an inf / NaN in B row J*bs + c reaches every row of every
 * block row that stores a block (I, J), whatever that block's column c holds.
 * Runs the full-panel kernels (bs 32 ROW blocks, row-major B: the LDS-staged
 * MFMA kernel the hybrid uses for dense blocks; otherwise the register-
 * fragment MFMA kernels) for spmm_bsrmm_ex_f32 / _f16, spmm_sbsrmm, the
 * analysed entries (which then ignore the masks) and the hybrid's BSR part.
 * Same result as the default on finite inputs, within the fp32 bar. */
#define SPMM_BSR_DENSE_BLOCK_PRODUCT 1
/* SPMM_BSR_SMALL_GROUPED: bs 2 / 4 / 8 (row-major B) take the grouped MFMA stream
 * (32 / bs block rows per wave share each B row of their column
 * union) whatever the matrix's size. By default it is taken from 2^20 stored
 * blocks up, where its fixed cost (a sharing probe and a block-row order,
 * about 40 us) is under a tenth of the product; below, and on matrices the probe
 * finds unshared, the lane-group VALU kernel runs. Same result bit for bit. */
#define SPMM_BSR_SMALL_GROUPED 2
spmm_status_t spmm_set_bsr_options(spmm_handle_t handle, int flags);

/* Which kernel the handle's last bs 2 / 4 / 8 fp32 product ran (a measurement
 * aid: the choice does not change the result): *path = 0 the lane-group VALU
 * kernel, 1 the grouped MFMA stream, 2 the grouped stream's branch whose
 * sharing probe gave the matrix to the lane-group kernel, -1 no such product
 * on this handle. Synchronises the handle's stream and reads the probe's sums
 * back; call it right after the product (the next product on the handle
 * reuses that scratch). */
spmm_status_t spmm_bsr_small_path(spmm_handle_t handle, int* path);

/* Build options of the loaded library (bit flags): SPMM_BUILD_TUNING is set
 * in an A/B build (make TUNING=1), whose kernel choice the environment may
 * override (SPMM_BSR_VARIANT, SPMM_BSR_ORDER, SPMM_CSR_GROUP_PD); a release
 * build reads no environment variable. */
#define SPMM_BUILD_TUNING 1
int spmm_get_build_options(void);

/* ------------------------------------------------------------------------ */
/* Path A: CSR x dense                                                         */
/* ------------------------------------------------------------------------ */

/* Drop-in for gespmm_csrmm<float> (gespmm_csrmm.h:422-426):
 *   C[A_nrows x B_ncols] = A(csr) * B, B and C row-major (ld = B_ncols),
 *   C overwritten (no alpha/beta), empty rows give 0. nnz is read from
 *   A_rowPtr[A_nrows] on the device. Runs on `stream` with a process-wide
 *   default handle. */
spmm_status_t spmm_gespmm_csrmm_f32(int A_nrows, int B_ncols, const int* A_rowPtr,
                                    const int* A_colInd, const float* A_val,
                                    const float* B, float* C, void* stream);

/* Drop-in for cusparseScsrmm (run_csrmm.cu:135-137):
 *   C(m x n, col-major, ldc) = alpha*op(A)(m x k) * B(k x n, col-major, ldb) + beta*C.
 * Only transA = NON_TRANSPOSE is supported (as in the reference call sites);
 * anything else returns SPMM_STATUS_MATRIX_TYPE_NOT_SUPPORTED, here and in
 * spmm_scsrmm2, spmm_dcsrmm2, spmm_sbsrmm and spmm_dbsrmm. For a transposed
 * product, build A^T once with spmm_csr2csc_dev and multiply by that. */
spmm_status_t spmm_scsrmm(spmm_handle_t handle, spmm_operation_t transA, int m, int n, int k,
                          int nnz, const float* alpha, const spmm_mat_descr_t descrA,
                          const float* csrValA, const int* csrRowPtrA, const int* csrColIndA,
                          const float* B, int ldb, const float* beta, float* C, int ldc);

/* Drop-in for cusparseScsrmm2 (run_csrmm.cu:139-142, test_csrmm.cu:126-129):
 *   transB = NON_TRANSPOSE: B col-major k x n (ldb >= k);
 *   transB = TRANSPOSE:     B row-major k x n (ldb >= n);  C col-major.
 * transA = NON_TRANSPOSE only; for A^T build it once with spmm_csr2csc_dev. */
spmm_status_t spmm_scsrmm2(spmm_handle_t handle, spmm_operation_t transA,
                           spmm_operation_t transB, int m, int n, int k, int nnz,
                           const float* alpha, const spmm_mat_descr_t descrA,
                           const float* csrValA, const int* csrRowPtrA,
                           const int* csrColIndA, const float* B, int ldb,
                           const float* beta, float* C, int ldc);

/* General form with explicit dense storage orders (host-pointer alpha/beta).
 *   C(m x n) = alpha * A(m x k, csr) * B(k x n) + beta * C
 * orderB/orderC = SPMM_ORDER_ROW is the fast (native) layout; column-major
 * operands are staged through the handle workspace. beta == 0 never reads C. */
spmm_status_t spmm_csrmm_ex_f32(spmm_handle_t handle, int m, int n, int k, int nnz,
                                float alpha, const int* csrRowPtr, const int* csrColInd,
                                const float* csrVal, spmm_index_base_t base,
                                const float* B, int ldb, spmm_order_t orderB, float beta,
                                float* C, int ldc, spmm_order_t orderC);

/* fp16 A values and B, fp32 accumulate, C, alpha and beta (fp16 as uint16_t bit
 * patterns, as in spmm_bsrmm_ex_f16): the checks, quick returns and ld rules of
 * spmm_csrmm_ex_f32 / spmm_gespmm_csrmm_f32, ldb counted in halves. binary16 widens
 * to binary32 exactly (subnormals included), so C is, bit for bit and signed zeros
 * included, what spmm_csrmm_ex_f32 gives on the widened inputs under
 * SPMM_CSR_SEQUENTIAL_ROWS: the piece association of the merge-path kernel at every n,
 * whatever the grid, the row shard, the entry point, the storage orders or B's
 * alignment (a B at an odd half offset or with an odd ldb is gathered one half per
 * lane). A column-major B is staged through the handle workspace in halves. */
spmm_status_t spmm_csrmm_ex_f16(spmm_handle_t handle, int m, int n, int k, int nnz,
                                float alpha, const int* csrRowPtr, const int* csrColInd,
                                const uint16_t* csrVal, spmm_index_base_t base,
                                const uint16_t* B, int ldb, spmm_order_t orderB, float beta,
                                float* C, int ldc, spmm_order_t orderC);
spmm_status_t spmm_gespmm_csrmm_f16(int A_nrows, int B_ncols, const int* A_rowPtr,
                                    const int* A_colInd, const uint16_t* A_val,
                                    const uint16_t* B, float* C, void* stream);

/* Hot-column analysis for the CSR gathers (an extension, once per matrix like
 * cuSPARSE's SpMM preprocess; the reference's gespmm_csrmm.h / csrmm.cu have
 * none). Counts every column's nonzeros on the device and writes
 *   csrColIndHot[i] = csrColInd[i] | 0x80000000  if column csrColInd[i] is hot,
 *                     csrColInd[i]               otherwise,
 * hot = among the columns with the most nonzeros whose gathered B-row pieces
 * (n floats, at most one merge-path column tile) fit in hotBytes (0 = the
 * default below: half the 256-MB MALL). Requires column indices < 2^31 - 1.
 * The piece size assumes 16-B aligned B and C with ld % 4 == 0 (the layout
 * the kernel gathers 2 or 4 floats per lane from); with a misaligned B the
 * kernel gathers one float per lane and the hot set is up to 4x smaller than
 * hotBytes (results are unaffected: the tags are cache hints only).
 * Caller-owned output (nnz ints); scratch comes from the handle. The tagged
 * array is input for spmm_csrmm_hot_f32 only: every other entry reads it as
 * negative (out-of-range) column indices. */
#define SPMM_CSR_HOT_BYTES_DEFAULT (128ll << 20)
spmm_status_t spmm_csr_hot_analysis(spmm_handle_t handle, int n, int k, int nnz,
                                    const int* csrColInd, spmm_index_base_t base,
                                    long long hotBytes, int* csrColIndHot);

/* spmm_csrmm_ex_f32 on the tagged column indices of spmm_csr_hot_analysis:
 * hot columns' B rows are gathered with the default cache policy, every other
 * row non-temporal, so the long tail of rarely used rows does not evict the hub
 * rows from L2 and the MALL. Same arithmetic, order and result as
 * spmm_csrmm_ex_f32 on the untagged indices (bit-identical), same checks. */
spmm_status_t spmm_csrmm_hot_f32(spmm_handle_t handle, int m, int n, int k, int nnz,
                                 float alpha, const int* csrRowPtr, const int* csrColIndHot,
                                 const float* csrVal, spmm_index_base_t base, const float* B,
                                 int ldb, spmm_order_t orderB, float beta, float* C, int ldc,
                                 spmm_order_t orderC);

/* ------------------------------------------------------------------------ */
/* Path B: BSR x dense                                                         */
/* ------------------------------------------------------------------------ */

/* Drop-in for cusparseSbsrmm (run_bsrmm.cu:160-165) and, with alpha/beta
 * passed by pointer, rocsparse_bsrmm_template<float> (rocsparse_bsrmm.h:102-108):
 *   C(mb*bs x n, col-major, ldc) = alpha * A(bsr, mb x kb blocks) * op(B) + beta * C
 *   dir: block storage (ROW: val[b*bs*bs + r*bs + c]; COLUMN: val[b*bs*bs + c*bs + r])
 *   transB = NON_TRANSPOSE: B col-major (kb*bs x n, ldb >= kb*bs)
 *   transB = TRANSPOSE:     B row-major (kb*bs x n, ldb >= n)
 * Status behaviour follows rocsparse_bsrmm.h:109-176 (NOT_INITIALIZED for a
 * null handle, INVALID_VALUE for null descr / negative sizes / null pointers /
 * bad ld, MATRIX_TYPE_NOT_SUPPORTED for transA != N or a bad transB, SUCCESS
 * quick return when mb, n, kb or nnzb is 0). For a transposed A, transpose the
 * CSR form once with spmm_csr2csc_dev and convert that (spmm_scsr2bsr_dev). */
spmm_status_t spmm_sbsrmm(spmm_handle_t handle, spmm_direction_t dir,
                          spmm_operation_t transA, spmm_operation_t transB, int mb, int n,
                          int kb, int nnzb, const float* alpha, const spmm_mat_descr_t descrA,
                          const float* bsrValA, const int* bsrRowPtrA, const int* bsrColIndA,
                          int blockDim, const float* B, int ldb, const float* beta, float* C,
                          int ldc);

/* General form with explicit dense storage orders.
 *   C(mb*bs x n) = alpha * A(bsr) * B(kb*bs x n) + beta * C
 * bs in {16, 32} runs on fp32 MFMA (v_mfma_f32_{16x16x4,32x32x2}_f32); other
 * block sizes run a VALU kernel. The per-block cublasSgemm variant of
 * block_cublas.cu:123-136 is dir = COLUMN, orderB = ROW, orderC = COL, beta = 1. */
spmm_status_t spmm_bsrmm_ex_f32(spmm_handle_t handle, spmm_direction_t dir, int mb, int kb,
                                int n, int nnzb, int blockDim, float alpha,
                                const int* bsrRowPtr, const int* bsrColInd,
                                const float* bsrVal, const float* B, int ldb,
                                spmm_order_t orderB, float beta, float* C, int ldc,
                                spmm_order_t orderC);

/* Analysis for the bs = 32 column stream (an extension: rocsparse_bsrmm.h:102-256
 * has no analysis step; this follows rocSPARSE's bsrmv analysis / cuSPARSE's
 * SpMM preprocess pattern). Once per matrix, on the handle's stream:
 *   masks[k]  bit c set iff column c of block k holds a value other than +-0
 *             (NaN and inf count), nnzb words;
 *   valCol    dir = ROW: a column-major copy of the blocks, nnzb * 1024 floats
 *             (may be null for dir = COLUMN, whose blocks already are).
 * Caller-owned buffers. bsrVal must be 16-byte aligned (the analysis reads
 * 16-B vectors). masks and valCol need only their element type's alignment
 * (4 bytes), here and in spmm_bsrmm_analysed_f32: the analysis writes them one
 * element at a time. The analysed stream, however, needs a 16-byte aligned
 * valCol; from any other valCol the product runs the generic kernel (one
 * element per load, the same result within the fp32 bar, far slower), so a
 * caller carving valCol out of an arena should place it on 16 bytes.
 * INVALID_VALUE for a bad dir, nnzb < 0, a null pointer that is needed, a
 * bsrVal off 16 bytes, or a valCol that overlaps bsrVal (the analysis
 * reads whole blocks while it scatters their columns: no in-place form). */
spmm_status_t spmm_bsr32_analysis_f32(spmm_handle_t handle, spmm_direction_t dir, int nnzb,
                                      const float* bsrVal, unsigned* masks, float* valCol);

/* C(mb*32 x n) = alpha * A * B(kb*32 x n) + beta * C on the analysis: valCol are
 * the column-major blocks (valCol from spmm_bsr32_analysis_f32, or bsrVal of a
 * COLUMN-direction matrix) and masks their column masks. A column of a block
 * with no value other than +-0 is skipped, as the shipped column streams do; the
 * kernel reads only the nonzero columns' values. Same checks and quick returns
 * as spmm_bsrmm_ex_f32 with blockDim 32; layouts the analysed kernel cannot
 * take run the COLUMN-direction kernels on valCol. */
spmm_status_t spmm_bsrmm_analysed_f32(spmm_handle_t handle, int mb, int kb, int n, int nnzb,
                                      float alpha, const int* bsrRowPtr, const int* bsrColInd,
                                      const float* valCol, const unsigned* masks, const float* B,
                                      int ldb, spmm_order_t orderB, float beta, float* C,
                                      int ldc, spmm_order_t orderC);

/* The same analysis for bs = 16 fp16 blocks: masks[k] bit c (c < 16), and for
 * ROW blocks a column-major fp16 copy (nnzb * 256 halves); same checks, with
 * bsrVal on 8 bytes. masks (4-byte words) and valCol (2-byte halves) again need
 * only their element alignment; a valCol off 16 bytes sends
 * spmm_bsrmm_analysed_f16 to the generic kernel. */
spmm_status_t spmm_bsr16_analysis_f16(spmm_handle_t handle, spmm_direction_t dir, int nnzb,
                                      const uint16_t* bsrVal, unsigned* masks, uint16_t* valCol);

/* C(mb*16 x n, fp32) = alpha * A * B(kb*16 x n, fp16) + beta * C on the bs = 16
 * analysis (fp16 A and B, fp32 accumulate), as spmm_bsrmm_ex_f16 with blockDim 16:
 * n >= 128 runs the analysed column stream, other shapes the COLUMN-direction
 * kernels on valCol. */
spmm_status_t spmm_bsrmm_analysed_f16(spmm_handle_t handle, int mb, int kb, int n, int nnzb,
                                      float alpha, const int* bsrRowPtr, const int* bsrColInd,
                                      const uint16_t* valCol, const unsigned* masks,
                                      const uint16_t* B, int ldb, spmm_order_t orderB,
                                      float beta, float* C, int ldc, spmm_order_t orderC);

/* The grouped bs = 16 fp16 stream (an extension, once per matrix like the
 * analyses above; DESIGN.md §4 "The grouped stream"). groupRows (2, 4 or 8;
 * 0 = the library's choice per matrix: the size query counts the items of
 * every W and keeps the one its time model ranks first, so a reordered graph
 * whose neighbouring rows share few columns gets 2; word 0 of the buffer holds
 * the W taken) adjacent block rows form a group whose waves share one copy of each
 * B row the union of their nonzero columns needs: on a reordered graph
 * neighbouring block rows need mostly the same rows (products stand-in: the
 * union is 0.43 of the (block row, column) pairs at 4 rows, 0.29 at 8).
 * Two phases: with buffer == NULL (the size query), *bufferBytes receives the
 * size of the caller-owned device buffer; with a buffer of that size the
 * analysis fills it. Everything runs on the device: the size query checks the
 * row pointer, counts and sums the groups' items there and synchronises the
 * handle's stream once (16 bytes come back for the size); the filling call
 * with the same arguments starts from the size query's device results, kept
 * on the handle, and only launches kernels and async copies (no
 * synchronisation, no host data: it can be captured in a HIP graph once the
 * handle's workspace has grown to the matrix). The arrays must not change
 * between the two calls (as between cuSPARSE's bufferSize and preprocess);
 * a filling call without a size query of the same arguments runs one first,
 * and every size query recomputes (a matrix at the addresses of an earlier
 * query is analysed afresh). Analyses on one handle from several threads run
 * one after the other (the handle's pending record is locked per call).
 * The handle records the buffer's layout:
 * spmm_bsrmm_grouped_f16 on the same handle takes it (until
 * spmm_bsr16_group_release or another analysis into the same buffer).
 * INVALID_VALUE for a bad dir / groupRows, negative sizes, null pointers that
 * are needed, a row pointer that does not run 0 .. nnzb, a negative block
 * column, block columns not strictly increasing within a block row (sorted,
 * no duplicates, as the csr2bsr output), a short buffer, a bsrVal off 8 bytes
 * (16 for spmm_bsr32_group_analysis_f32) or a buffer that is not 16-byte
 * aligned (its sections, at multiples of 256 bytes from its start, are read
 * and written as 16-byte vectors; the status comes before any launch and the
 * buffer is not touched); NOT_SUPPORTED past 2^31 - 1 items. */
spmm_status_t spmm_bsr16_group_analysis_f16(spmm_handle_t handle, spmm_direction_t dir, int mb,
                                            int nnzb, int groupRows, const int* bsrRowPtr,
                                            const int* bsrColInd, const uint16_t* bsrVal,
                                            void* buffer, size_t* bufferBytes);

/* C(mb*16 x n, fp32) = alpha * A * B(kb*16 x n, fp16) + beta * C on a group
 * analysis of A (fp32 accumulate), B row- or column-major (staged row-major),
 * C either order. Same sizes and ld checks as spmm_bsrmm_ex_f16;
 * INVALID_VALUE for a buffer this handle has no analysis of, another mb, or a
 * kb the analysed block columns do not fit (a column >= kb);
 * NOT_SUPPORTED when n % 8 != 0, a row-major ldb % 8 != 0 or B is not 16-B
 * aligned (spmm_bsrmm_ex_f16 serves those shapes). Non-finite B follows the
 * column-granular contract of the drop-in stream (spmm_set_bsr_options above):
 * each wave clears the B values of the entries its block row does not hold;
 * with finite B the product equals spmm_bsrmm_ex_f16's within the fp32 bar. */
spmm_status_t spmm_bsrmm_grouped_f16(spmm_handle_t handle, int mb, int kb, int n,
                                     const void* buffer, float alpha, const uint16_t* B, int ldb,
                                     spmm_order_t orderB, float beta, float* C, int ldc,
                                     spmm_order_t orderC);
/* The grouped bs = 32 fp32 stream (an extension, like the bs 16 one above;
 * DESIGN.md §4 "The grouped bs 32 stream"). groupRows 2 or 4 (0 = 2) adjacent
 * block rows share one copy of each B row of their union; unlike bs 16 each
 * block row multiplies only its own nonzero columns (the analysis records them
 * per item), so C is bit-identical to spmm_bsrmm_ex_f32 /
 * spmm_bsrmm_analysed_f32 with the same column-granular non-finite contract
 * (on every block row that those do not split: with a row-major C on a grid of
 * few block rows they cut a block row far longer than the others into segments
 * and add the segments' partial sums, which the grouped stream never does;
 * such a row agrees within the fp32 bar).
 * Same two phases, checks and handle record as spmm_bsr16_group_analysis_f16.
 * The analysis reads A once: for ROW blocks the size query keeps a compact copy
 * of the blocks' nonzero columns in a stream-ordered allocation of 4 KB per block
 * (at most 16 GiB and a quarter of the free device memory)
 * (hipMallocAsync on the handle's stream), which the filling call reads and frees;
 * a filling call under stream capture reads the values instead and leaves the
 * copy to the next size query or spmm_destroy. Without memory for the copy the
 * filling call reads the blocks themselves; the buffer's bytes are the same. */
spmm_status_t spmm_bsr32_group_analysis_f32(spmm_handle_t handle, spmm_direction_t dir, int mb,
                                            int nnzb, int groupRows, const int* bsrRowPtr,
                                            const int* bsrColInd, const float* bsrVal,
                                            void* buffer, size_t* bufferBytes);

/* C(mb*32 x n) = alpha * A * B(kb*32 x n) + beta * C on a bs 32 group analysis of A,
 * B and C row- or column-major (column-major ones are staged row-major in the
 * workspace). INVALID_VALUE as spmm_bsrmm_grouped_f16 (a bs 16 analysis is not
 * taken); NOT_SUPPORTED when n % 4 != 0, a row-major ldb or ldc % 4 != 0, or B or
 * C is not 16-B aligned (spmm_bsrmm_ex_f32 serves those shapes). */
spmm_status_t spmm_bsrmm_grouped_f32(spmm_handle_t handle, int mb, int kb, int n,
                                     const void* buffer, float alpha, const float* B, int ldb,
                                     spmm_order_t orderB, float beta, float* C, int ldc,
                                     spmm_order_t orderC);

/* Forgets the handle's record of a group-analysis buffer, bs 16 or bs 32 (before
 * freeing it). spmm_bsr_group_release is the same call under a block-size-neutral
 * name; spmm_bsr16_group_release stays for the bs 16 stream's first users. */
spmm_status_t spmm_bsr_group_release(spmm_handle_t handle, const void* buffer);
spmm_status_t spmm_bsr16_group_release(spmm_handle_t handle, const void* buffer);

/* fp16 A and B (IEEE binary16 bit patterns), fp32 accumulate and fp32 C.
 * bs = 16 runs on v_mfma_f32_16x16x32_f16 with two blocks per instruction. */
spmm_status_t spmm_bsrmm_ex_f16(spmm_handle_t handle, spmm_direction_t dir, int mb, int kb,
                                int n, int nnzb, int blockDim, float alpha,
                                const int* bsrRowPtr, const int* bsrColInd,
                                const uint16_t* bsrVal, const uint16_t* B, int ldb,
                                spmm_order_t orderB, float beta, float* C, int ldc,
                                spmm_order_t orderC);

/* Re-blocking to bs 32 on the device (an extension; DESIGN.md §4, "Small blocks
 * re-blocked to 32"): the same matrix in 32 x 32 blocks, so a bs = 2 / 4 / 8 / 16
 * product can run on the bs 32 MFMA streams (spmm_bsr32_analysis_f32 +
 * spmm_bsrmm_analysed_f32, or the group analysis) instead of the VALU kernel.
 * A block (I, J) of blockDim lands in block (I / R, J / R), R = 32 / blockDim, at
 * sub-block (I % R, J % R); the rest of each 32 x 32 block is zero. dir is kept
 * (ROW blocks stay ROW). mb32 = ceil(mb / R) block rows; the product then needs
 * B with ceil(kb / R) * 32 rows and C with mb32 * 32 rows (the extra rows are
 * zero columns / rows of A). cusparseXcsr2bsrNnz / Scsr2bsr's two calls: the
 * first fills bsrRowPtr32[mb32 + 1] and *nnzb32HostPtr (it synchronises the
 * handle's stream), the second bsrColInd32[nnzb32] and bsrVal32[nnzb32 * 1024]
 * (zero-filled first; no synchronisation). Block columns must be sorted per
 * block row; a negative one is INVALID_VALUE. */
spmm_status_t spmm_xbsr_reblock32_nnzb(spmm_handle_t handle, spmm_direction_t dir, int mb,
                                       int nnzb, int blockDim, const int* bsrRowPtr,
                                       const int* bsrColInd, int* bsrRowPtr32,
                                       int* nnzb32HostPtr);
spmm_status_t spmm_sbsr_reblock32(spmm_handle_t handle, spmm_direction_t dir, int mb, int nnzb,
                                  int blockDim, const int* bsrRowPtr, const int* bsrColInd,
                                  const float* bsrVal, const int* bsrRowPtr32, int nnzb32,
                                  int* bsrColInd32, float* bsrVal32);

/* ------------------------------------------------------------------------ */
/* Preprocessing on the HOST (all pointers are host pointers)                  */
/* ------------------------------------------------------------------------ */

/* cusparseXcsr2bsrNnz semantics (run_bsrmm.cu:121-131): fills
 * bsrRowPtr[mb+1] (mb = ceil(m/blockDim)) and *nnzbTotal. */
spmm_status_t spmm_xcsr2bsr_nnz(spmm_direction_t dir, int m, int n, const int* csrRowPtr,
                                const int* csrColInd, int blockDim, int* bsrRowPtr,
                                int* nnzbTotal);

/* cusparseScsr2bsr semantics (run_bsrmm.cu:136-142): bsrRowPtr must come from
 * spmm_xcsr2bsr_nnz; bsrColInd[nnzb] sorted per block row; bsrVal[nnzb*bs*bs]
 * zero-filled, values placed per `dir`. Duplicate (row, col) entries are
 * summed. */
spmm_status_t spmm_scsr2bsr(spmm_direction_t dir, int m, int n, const float* csrVal,
                            const int* csrRowPtr, const int* csrColInd, int blockDim,
                            const int* bsrRowPtr, float* bsrVal, int* bsrColInd);

/* CSR -> CSC, that is the CSR form of A^T (n x m); no reference counterpart.
 *   Input: csrRowPtr[m + 1], csrColInd, csrVal in baseA; nnz = csrRowPtr[m] -
 *     csrRowPtr[0]. csrRowPtr[0] need not be the base (a view into a larger
 *     matrix): position p is index p of csrColInd / csrVal as passed, and the
 *     matrix holds the positions from csrRowPtr[0] - baseA on. Rows need not be
 *     sorted by column.
 *   Output: cscColPtr[n + 1] (cscColPtr[0] = baseC, cscColPtr[n] = nnz + baseC,
 *     a column without entries repeats the pointer), cscRowInd[nnz] in baseC,
 *     cscVal[nnz] and, when perm is not NULL, perm[nnz] = the CSR position of
 *     each CSC entry (0-based; cscVal = csrVal[perm] refreshes the values of a
 *     matrix whose pattern stays). Inside a column the entries are in ascending
 *     CSR position (ascending row; duplicate (row, col) entries keep their CSR
 *     order): the stable sort of the positions by column, so every output byte
 *     is a function of the input alone, and the output's rows are sorted by
 *     column whatever the input's were.
 *   valueBytes = 0 (pattern only; csrVal / cscVal may be NULL), 2, 4 or 8: the
 *     values are moved as opaque words (binary16, fp32, fp64).
 *   Input and output arrays must not overlap.
 *   SPMM_STATUS_INVALID_VALUE: a negative size, another valueBytes or base, a
 *     needed pointer that is NULL, a decreasing row pointer, csrRowPtr[0] below
 *     baseA, an nnz other than the row pointer's, a column outside [0, n).
 * Host pointers, worker threads like the other host conversions. */
spmm_status_t spmm_csr2csc(int m, int n, int nnz, const void* csrVal, const int* csrRowPtr,
                           const int* csrColInd, int valueBytes, spmm_index_base_t baseA,
                           spmm_index_base_t baseC, void* cscVal, int* cscColPtr,
                           int* cscRowInd, int* perm);

/* cusparseSbsr2csr semantics (bsr2csr.cu:177-188): every block expanded,
 * explicit zeros kept: nnz = nnzb*bs*bs, csrRowPtr[mb*bs+1]. */
spmm_status_t spmm_sbsr2csr(spmm_direction_t dir, int mb, int nb, const float* bsrVal,
                            const int* bsrRowPtr, const int* bsrColInd, int blockDim,
                            float* csrVal, int* csrRowPtr, int* csrColInd);

/* calculateNnzb (utility.cc:47-69) over a CSR pattern: number of nonzero
 * bs x bs blocks. */
int64_t spmm_calculate_nnzb(int n, const int* csrRowPtr, const int* csrColInd, int blockDim);

/* nnz-balanced contiguous row partition for multi-GPU sharding:
 * bounds[0] = 0, bounds[nparts] = m, part p owns rows [bounds[p], bounds[p+1]).
 * Minimises the max over parts of (nnz + rows) by a prefix search on rowptr. */
spmm_status_t spmm_csr_partition_rows(int m, const int* csrRowPtr, int nparts, int* bounds);

/* divide_matrix (divide.cu:52-127), with values: the n x n CSR is split into
 * a BSR part (DIRECTION_ROW) holding every bs x bs block whose fill
 * (entries / bs^2) is >= density, and a CSR remainder holding the other
 * entries in their original order. As in the reference, density <= 0 admits
 * every block, empty ones included (divide.cu:91). Host pointers, two
 * phases: sizes (csrRowPtr[n+1], bsrRowPtr[mb+1], totals), then fill.
 * Duplicate entries inside a BSR block are summed. */
spmm_status_t spmm_divide_nnz(int n, const int* rowPtr, const int* colInd, int blockDim,
                              float density, int* csrRowPtr, int* bsrRowPtr, int* csrNnz,
                              int* nnzb);
spmm_status_t spmm_sdivide(int n, const int* rowPtr, const int* colInd, const float* val,
                           int blockDim, float density, const int* csrRowPtr,
                           const int* bsrRowPtr, int* csrColInd, float* csrVal, int* bsrColInd,
                           float* bsrVal);

/* Device-pointer conversions: the argument order and
 * meaning of cusparseXcsr2bsrNnz / cusparseScsr2bsr (run_bsrmm.cu:121-142) and
 * cusparseSbsr2csr (bsr2csr.cu:186-188), on the handle's stream. The index
 * bases come from the descriptors. csr2bsr needs rows sorted by column (the
 * csrSorted* contract) and blockDim <= 64; duplicates are summed in CSR
 * order, so every output is bit-identical to the host conversions above.
 * nnzTotalHostPtr is a host pointer (the call synchronises, as cuSPARSE's host
 * pointer mode does); a column outside [0, n) makes it return
 * SPMM_STATUS_INVALID_VALUE. csr2bsr zero-fills bsrVal itself. */
spmm_status_t spmm_xcsr2bsr_nnz_dev(spmm_handle_t handle, spmm_direction_t dir, int m, int n,
                                    const spmm_mat_descr_t descrA, const int* csrRowPtr,
                                    const int* csrColInd, int blockDim,
                                    const spmm_mat_descr_t descrC, int* bsrRowPtr,
                                    int* nnzTotalHostPtr);
spmm_status_t spmm_scsr2bsr_dev(spmm_handle_t handle, spmm_direction_t dir, int m, int n,
                                const spmm_mat_descr_t descrA, const float* csrVal,
                                const int* csrRowPtr, const int* csrColInd, int blockDim,
                                const spmm_mat_descr_t descrC, float* bsrVal,
                                const int* bsrRowPtr, int* bsrColInd);
spmm_status_t spmm_sbsr2csr_dev(spmm_handle_t handle, spmm_direction_t dir, int mb, int nb,
                                const spmm_mat_descr_t descrA, const float* bsrVal,
                                const int* bsrRowPtr, const int* bsrColInd, int blockDim,
                                const spmm_mat_descr_t descrC, float* csrVal, int* csrRowPtr,
                                int* csrColInd);

/* spmm_csr2csc on the device: the contract of spmm_csr2csc above, bit for bit
 * (tests/test_gpu_csr2csc.py), device pointers, the handle's stream, the index
 * bases from the descriptors. A column-count histogram (integer atomics: a
 * count does not depend on arrival order), then a stable LSD radix sort of the
 * positions by column in ceil(bits(n - 1) / 8) passes of 8-bit digits whose
 * ranks come from ballots and scans, never from an atomic, then one gather of
 * rows (written out per position once) and values: no per-column work, so a hub column
 * costs what its entries cost anywhere else.
 *   Checks, in order: a NULL handle is SPMM_STATUS_NOT_INITIALIZED; then the
 *     host-side SPMM_STATUS_INVALID_VALUE cases of spmm_csr2csc that need no
 *     data (sizes, valueBytes, NULL descriptors or pointers, nnz > 0 with
 *     n = 0); under stream capture SPMM_STATUS_NOT_SUPPORTED before anything
 *     is queued; nnz = 0 fills cscColPtr with baseC and returns.
 *   A column outside [0, n), a decreasing row pointer or an nnz other than the
 *     row pointer's is found on the device (such an entry is skipped, never
 *     used as an index) and reported as SPMM_STATUS_INVALID_VALUE after the
 *     call's one synchronisation, before anything is sorted; the outputs are
 *     then unspecified. Because of that read-back the call cannot be captured.
 *   Workspace: from the handle (a steady-state repeat allocates nothing): 4 n
 *     bytes of column counts plus at most 20.25 bytes per nonzero: 4 for the
 *     row of every position, 0.25 for the tile counts and their scan, and two
 *     key and two position buffers of 4 each from three passes on (n > 65 536).
 *     Two passes: 16.25, 12.25 with perm (the last pass writes into it); one
 *     pass: 8.25, 4.25 with perm; n <= 1: 4. With kernel timing on, every
 *     kernel of the call is timed: count, scan, then (digit count, scan,
 *     scatter) per pass, then the row expansion and the gather. */
spmm_status_t spmm_csr2csc_dev(spmm_handle_t handle, int m, int n, int nnz,
                               const spmm_mat_descr_t descrA, const void* csrVal,
                               const int* csrRowPtr, const int* csrColInd, int valueBytes,
                               const spmm_mat_descr_t descrC, void* cscVal, int* cscColPtr,
                               int* cscRowInd, int* perm);

/* CSR-sampled dense-dense product (SDDMM, cusparseSDDMM's shape; no reference
 * counterpart): for every position p of the m x k CSR pattern
 *     outVal[p] = epi(dot(X[i(p), 0..n), Y[j(p), 0..n)))
 * with i(p) the row that holds p and j(p) = csrColInd[p] - base; epi(d) = alpha * d
 * when beta == 0 (outVal is then never read), else fma(beta, outVal[p], alpha * d),
 * the epilogue of the CSR products. With X = grad_C and Y = B it is the gradient of
 * A's values in C = A * B; with X = Y = H the edge logits <h_i, h_j> of a graph.
 *   X is m x n and Y is k x n, row-major fp32, ldx, ldy >= n counted in floats; X and
 *     Y may be the same buffer. n = 0 is valid: the dot is +0.
 *   csrColInd and outVal hold nnz entries and share their index: position p is index
 *     p of both as passed, and the pattern holds the positions csrRowPtr[0] - base ..
 *     csrRowPtr[m] - base (csrRowPtr[0] may exceed the base, as in spmm_csr2csc: a
 *     view into a larger matrix; entries outside the view are left alone). Duplicate
 *     (row, col) entries and rows not sorted by column are ordinary input.
 *   The association rule: the bits of outVal[p] depend on the two rows, n, alpha,
 *     beta and the old outVal[p] alone, never on the grid or the worker count, on
 *     p's place in the array, on the row's length, on ldx / ldy or the operands'
 *     alignment, or on the entry point (device = host, bit for bit).
 *       G(n) = min(64, max(1, pow2ceil(ceil(n / 4)))) chains make one dot. Chain l
 *       owns the columns c with (c / 4) mod G == l and sums them in ascending c as
 *       acc = fma(x[c], y[c], acc) in fp32, starting from +0 (a chain without a
 *       column stays +0). The chains fold in the butterfly acc_l + acc_(l xor s) for
 *       s = 1, 2, ..., G / 2, that is pairwise over adjacent chains, level by level.
 *       On the device a chain is a lane (64 / G positions per wave instruction); a
 *       base that is not 16-byte aligned or an ld with ld % 4 != 0 changes how a
 *       lane's words are loaded (single dwords instead of dwordx4), not which lane
 *       sums them: the policy of the fp16 CSR entries.
 *   Checks, in order: negative m, n, k or nnz, another base, ldx < n or ldy < n, or
 *     a NULL pointer with nnz > 0 (X and Y only when n > 0) are
 *     SPMM_STATUS_INVALID_VALUE; m == 0 or nnz == 0 returns success at once. The host
 *     form also refuses (before it writes anything) a decreasing row pointer,
 *     csrRowPtr[0] below the base, csrRowPtr[m] - base above nnz and a column
 *     outside [0, k).
 * Host pointers, worker threads like the other host conversions. */
spmm_status_t spmm_sddmm_csr_host_f32(int m, int n, int k, int nnz, float alpha,
                                      const int* csrRowPtr, const int* csrColInd,
                                      spmm_index_base_t base, const float* X, int ldx,
                                      const float* Y, int ldy, float beta, float* outVal);

/* spmm_sddmm_csr_host_f32 on the device: the same contract and the same bits
 * (tests/test_gpu_sddmm.py), device pointers, one kernel on the handle's stream
 * (csrc/sddmm_kernels.hip). Every wave takes an equal share of the
 * positions, so degree skew costs nothing; a lane group keeps its row's X slice in
 * registers along a CSR row and has several Y-row gathers in flight.
 *   A NULL handle is SPMM_STATUS_NOT_INITIALIZED before the checks above. A column
 *     outside [0, k) or a bad row pointer is the caller's fault, as in
 *     spmm_csrmm_ex_f32: there is no device-side validation and no read-back (the
 *     positions are only ever clamped to [0, nnz), the rows to [0, m)).
 *   The call does not synchronise, takes nothing from the handle's buffers (a
 *     repeat allocates nothing, and it disturbs no other entry's state) and may be
 *     captured into a graph; a replay re-reads the pattern, X, Y and outVal at the
 *     captured addresses. With kernel timing on, its one kernel is timed. */
spmm_status_t spmm_sddmm_csr_f32(spmm_handle_t handle, int m, int n, int k, int nnz, float alpha,
                                 const int* csrRowPtr, const int* csrColInd,
                                 spmm_index_base_t base, const float* X, int ldx, const float* Y,
                                 int ldy, float beta, float* outVal);

/* Edge softmax (DGL's edge_softmax, PyG's softmax(src, ptr=...); no reference
 * counterpart): the softmax of x over the positions of every CSR row, the second step
 * of graph attention between spmm_sddmm_csr_f32 (the logits) and the CSR product on
 * those values. For every row r with the positions [a, b) = [csrRowPtr[r],
 * csrRowPtr[r + 1]) - base:
 *     mx   = max of x[a..b)              (fmaxf: a NaN operand is dropped)
 *     t[p] = x[p] - mx                   (one fp32 subtraction)
 *     e[p] = EXP(t[p])
 *     s    = SUM(e[a..b))
 *     y[p] = e[p] / s                    (IEEE fp32 division)
 * and the backward, from y and g = dloss/dy:
 *     d     = SUM over the row of y[p] * g[p], each chain acc = fma(y[p], g[p], acc)
 *     gx[p] = y[p] * (g[p] - d)          (the difference and the product rounded apart)
 *   x, y (g, gx) hold nnz floats and share the pattern's index, as csrColInd and outVal
 *     of spmm_sddmm_csr_f32 do; csrRowPtr[0] may exceed the base (a view): positions
 *     outside [csrRowPtr[0], csrRowPtr[m]) - base are never written. Empty rows write
 *     nothing. The column indices are not needed.
 *   The rule: the bits of a row's outputs depend on the row's own values alone, never
 *     on the grid, the worker count, the row's place, the other rows, a setting of the
 *     handle or the entry point (device = host, bit for bit).
 *       EXP (csrc/softmax_rule.hpp, one text for host and device): NaN -> NaN;
 *       t < -64 (-inf included) -> exactly +0; t == 0 -> exactly 1.0f; otherwise
 *       k = rint(t * log2(e)), r = fma(k, -ln2_lo, fma(k, -ln2_hi, t)), a degree-7 Horner
 *       polynomial of exp(r) in FMAs, and the scaling by 2^k on the exponent bits. Only
 *       fp32 +, *, FMA, rint, conversions and integer operations: no libm exp, no
 *       hardware approximation. Every nonzero term is a normal number, and so is every
 *       nonzero quotient, so no result depends on a denormal mode.
 *       SUM: the row is cut into pieces of 1024 positions counted from its start. In a
 *       piece, chain c (0 .. 63) takes the positions = c (mod 64) in ascending order,
 *       starting from +0; the 64 chains fold in the butterfly acc_l + acc_(l xor s),
 *       s = 1, 2, ..., 32 (pairwise over adjacent chains, level by level); the piece
 *       sums are added one after the other in ascending order, starting from +0. A row
 *       of at most 64 positions is a pairwise tree over its terms padded with +0.
 *   Special values follow from the rule: a NaN, a +inf or nothing but -inf in a row
 *     makes every output of that row NaN; a -inf (or anything more than 64 below the
 *     maximum) beside finite values gives exactly +0; a row of one finite value gives
 *     exactly 1.0f.
 *   Aliasing: y may be exactly x, gx may be exactly g; any other overlap is the
 *     caller's fault.
 *   Checks, in order: negative m or nnz, another base, or a NULL pointer with nnz > 0
 *     are SPMM_STATUS_INVALID_VALUE; m == 0 or nnz == 0 returns success at once. The
 *     host forms also refuse (before they write anything) a decreasing row pointer,
 *     csrRowPtr[0] below the base and csrRowPtr[m] - base above nnz.
 * Host pointers, worker threads like the other host conversions. */
spmm_status_t spmm_edge_softmax_csr_host_f32(int m, int nnz, const int* csrRowPtr,
                                             spmm_index_base_t base, const float* x, float* y);
spmm_status_t spmm_edge_softmax_bwd_csr_host_f32(int m, int nnz, const int* csrRowPtr,
                                                 spmm_index_base_t base, const float* y,
                                                 const float* g, float* gx);

/* The two host forms on the device: the same contract and the same bits
 * (tests/test_gpu_edge_softmax.py), device pointers, one kernel on the handle's stream
 * (csrc/softmax_kernels.hip). Waves take equal shares of the merge path
 * of rows and positions; lane groups of 4, 16 or 64 lanes (by the mean row length) take
 * a row of up to 1024 positions each, and a longer row is done by the one workgroup
 * that owns it, its pieces spread over that workgroup's waves. No workgroup waits for
 * another; there are no atomics.
 *   A NULL handle is SPMM_STATUS_NOT_INITIALIZED before the checks above. A bad row
 *     pointer is the caller's fault: there is no device-side validation and no
 *     read-back (positions are clamped to [0, nnz], rows to [0, m)).
 *   The calls do not synchronise, take nothing from the handle's buffers (a repeat
 *     allocates nothing) and may be captured into a graph; a replay re-reads the row
 *     pointer and the values at the captured addresses. With kernel timing on, the
 *     kernel is timed; with the launch record on, it is recorded. */
spmm_status_t spmm_edge_softmax_csr_f32(spmm_handle_t handle, int m, int nnz,
                                        const int* csrRowPtr, spmm_index_base_t base,
                                        const float* x, float* y);
spmm_status_t spmm_edge_softmax_bwd_csr_f32(spmm_handle_t handle, int m, int nnz,
                                            const int* csrRowPtr, spmm_index_base_t base,
                                            const float* y, const float* g, float* gx);

/* The three ops of a graph attention layer over `heads` heads in one call each (no
 * reference counterpart; csrc/heads_kernels.hip): the sampled product
 * (the logits), the edge softmax with its backward, and the CSR product on per-head
 * values. They replace the loop over heads of the single-head entries above and take the
 * layouts graph frameworks use:
 *   per-edge values (outVal, x, y, g, gx, csrVal): fp32 [nnz, heads], contiguous, element
 *     (p, h) at p * heads + h, p the position as in the single-head entries (the same
 *     base, the same csrRowPtr[0] > base views, the same clamping on the device);
 *   per-node features (X, Y, B, C): row-major [rows, ld], ld >= heads * d counted in
 *     floats, head h in the columns [h d, (h + 1) d): a contiguous [rows, heads, d].
 * The contract is per head the written rule of the single-head entry, bit for bit:
 *   spmm_sddmm_csr_heads_*: outVal[p, h] has the bits of spmm_sddmm_csr_f32 with n = d on
 *     X + h d, Y + h d and the same ldx / ldy (G(d) chains and their butterfly). It does
 *     not depend on alignment, ld, the grid or heads.
 *   spmm_edge_softmax_csr_heads_* / _bwd_: column h of the result has the bits of
 *     spmm_edge_softmax_csr_f32 / _bwd_csr_f32 on column h of the input (EXP, pieces of
 *     1024, 64 chains, butterfly). Heads never mix: a row made non-finite in head h
 *     leaves the other heads' bits alone. y may be exactly x, gx may be exactly g.
 *   spmm_csrmm_heads_*: C[i, h d + c] = epi(sum over the row's positions p of
 *     csrVal[p, h] * B[col(p), h d + c]) under the piece rule of the CSR product
 *     (DESIGN.md §3c), at every d: the row's L nonzeros are cut into pieces of
 *     max(128, ceil(L / 64)) nonzeros from its start, each piece a sequential chain
 *     acc = fma(val, b, acc) from +0, the pieces added left to right from -0 (an empty
 *     row is +0), then alpha * x, or fma(beta, C, alpha * x) when beta != 0. These are
 *     the bits of spmm_csrmm_ex_f32 under SPMM_CSR_SEQUENTIAL_ROWS on (csrVal[:, h],
 *     B[:, h d .. (h + 1) d)). Row-major B and C only. Sums start from +0, subnormals
 *     are kept, and a non-finite csrVal[p, h] or B element reaches exactly the outputs
 *     that reference it.
 *   heads = 1 equals the single-head entries bit for bit (the product: under
 *     SPMM_CSR_SEQUENTIAL_ROWS).
 * Checks: those of the single-head entry of each op in its order (spmm_csrmm_ex_f32's for
 *   the product, with ldb, ldc >= heads * d), and
 *     heads < 1                    SPMM_STATUS_INVALID_VALUE, with the negative sizes;
 *     nnz * heads > INT_MAX        SPMM_STATUS_NOT_SUPPORTED;
 *     d > 1024 (sampled product)   SPMM_STATUS_NOT_SUPPORTED (loop over column blocks of
 *                                  the single-head entry instead);
 *     heads * d > 65535 * 64 (device product)
 *                                  SPMM_STATUS_NOT_SUPPORTED (the column tiles of 64 are one
 *                                  extent of the grid);
 *   the two after the quick returns (m == 0 or nnz == 0; the product: m == 0 or d == 0)
 *   and before anything is read or queued.
 * The _host_ forms take host pointers and state the rules in executable form (worker
 *   threads like the other host conversions); they also refuse a decreasing row pointer,
 *   csrRowPtr[0] below the base, csrRowPtr[m] - base above nnz and, where there are column
 *   indices, a column outside [0, k). The device forms equal them bit for bit
 *   (tests/test_gpu_heads.py): a NULL handle is SPMM_STATUS_NOT_INITIALIZED before the
 *   other checks; there is no device-side validation (positions are clamped to [0, nnz],
 *   rows to [0, m)); each is one kernel on the handle's stream, takes nothing from the
 *   handle's buffers, uses no atomics, does not synchronise or read back, and may be
 *   captured into a graph. spmm_set_csr_waves_per_cu sizes the grids of all four; no grid
 *   changes a bit. A row of more than 1024 positions (softmax) or
 *   128 nonzeros (product) is done by the one workgroup that owns it. */
spmm_status_t spmm_sddmm_csr_heads_host_f32(int m, int d, int k, int nnz, int heads, float alpha,
                                            const int* csrRowPtr, const int* csrColInd,
                                            spmm_index_base_t base, const float* X, int ldx,
                                            const float* Y, int ldy, float beta, float* outVal);
spmm_status_t spmm_sddmm_csr_heads_f32(spmm_handle_t handle, int m, int d, int k, int nnz,
                                       int heads, float alpha, const int* csrRowPtr,
                                       const int* csrColInd, spmm_index_base_t base,
                                       const float* X, int ldx, const float* Y, int ldy,
                                       float beta, float* outVal);
spmm_status_t spmm_edge_softmax_csr_heads_host_f32(int m, int nnz, int heads,
                                                   const int* csrRowPtr, spmm_index_base_t base,
                                                   const float* x, float* y);
spmm_status_t spmm_edge_softmax_csr_heads_f32(spmm_handle_t handle, int m, int nnz, int heads,
                                              const int* csrRowPtr, spmm_index_base_t base,
                                              const float* x, float* y);
spmm_status_t spmm_edge_softmax_bwd_csr_heads_host_f32(int m, int nnz, int heads,
                                                       const int* csrRowPtr,
                                                       spmm_index_base_t base, const float* y,
                                                       const float* g, float* gx);
spmm_status_t spmm_edge_softmax_bwd_csr_heads_f32(spmm_handle_t handle, int m, int nnz, int heads,
                                                  const int* csrRowPtr, spmm_index_base_t base,
                                                  const float* y, const float* g, float* gx);
spmm_status_t spmm_csrmm_heads_host_f32(int m, int d, int k, int nnz, int heads, float alpha,
                                        const int* csrRowPtr, const int* csrColInd,
                                        const float* csrVal, spmm_index_base_t base,
                                        const float* B, int ldb, float beta, float* C, int ldc);
spmm_status_t spmm_csrmm_heads_f32(spmm_handle_t handle, int m, int d, int k, int nnz, int heads,
                                   float alpha, const int* csrRowPtr, const int* csrColInd,
                                   const float* csrVal, spmm_index_base_t base, const float* B,
                                   int ldb, float beta, float* C, int ldc);

/* The multi-head sampled product and product on fp16 and bf16 per-node features (no
 * reference counterpart; csrc/heads_half_kernels.hip). The arguments are
 * those of spmm_sddmm_csr_heads_f32 / spmm_csrmm_heads_f32, with X, Y / B given as 16-bit
 * patterns (IEEE binary16 for _f16, bfloat16 for _bf16, as in spmm_csrmm_ex_f16) and ldx,
 * ldy / ldb >= heads * d counted in elements. Edge values (outVal, csrVal), alpha, beta, C
 * and ldc stay fp32: the weights come from the fp32 edge softmax, which has no half form.
 * Contract: outVal / C equal, bit for bit and signed zeros included, what the _f32 entry
 *   gives on the operands widened to fp32 (both widenings are exact, subnormals included;
 *   nothing is flushed): the G(d) chains and butterfly for the sampled product, the piece
 *   rule at every d for the product. The bits do not depend on the grid, ld, alignment,
 *   heads, the vector width or the load path: a base that is only 2- or 4-byte aligned, or
 *   an odd ld, takes narrower loads and gives the same bits. A non-finite feature reaches
 *   exactly the outputs that reference it.
 * Everything else is the _f32 entries': the checks, their order, the quick returns and the
 *   refusals (heads < 1; nnz * heads > INT_MAX; d > 1024 for the sampled product;
 *   heads * d > 65535 * 64 for the device product); heads = 1 serves one head; the device
 *   entries queue one kernel on the handle's stream, take nothing from the handle's
 *   buffers, use no atomics, do not synchronise and may be captured;
 *   spmm_set_csr_waves_per_cu sizes the grids. The _host_ forms widen the operands and run
 *   the fp32 host forms, so they state the rule in executable form and refuse what those
 *   refuse.
 * Speed: DESIGN.md §4k's table (profiles/heads_half/summary.json); the gathered bytes per
 *   nonzero and head go from 4 d to 2 d. */
spmm_status_t spmm_sddmm_csr_heads_host_f16(int m, int d, int k, int nnz, int heads, float alpha,
                                            const int* csrRowPtr, const int* csrColInd,
                                            spmm_index_base_t base, const uint16_t* X, int ldx,
                                            const uint16_t* Y, int ldy, float beta, float* outVal);
spmm_status_t spmm_sddmm_csr_heads_host_bf16(int m, int d, int k, int nnz, int heads, float alpha,
                                             const int* csrRowPtr, const int* csrColInd,
                                             spmm_index_base_t base, const uint16_t* X, int ldx,
                                             const uint16_t* Y, int ldy, float beta,
                                             float* outVal);
spmm_status_t spmm_sddmm_csr_heads_f16(spmm_handle_t handle, int m, int d, int k, int nnz,
                                       int heads, float alpha, const int* csrRowPtr,
                                       const int* csrColInd, spmm_index_base_t base,
                                       const uint16_t* X, int ldx, const uint16_t* Y, int ldy,
                                       float beta, float* outVal);
spmm_status_t spmm_sddmm_csr_heads_bf16(spmm_handle_t handle, int m, int d, int k, int nnz,
                                        int heads, float alpha, const int* csrRowPtr,
                                        const int* csrColInd, spmm_index_base_t base,
                                        const uint16_t* X, int ldx, const uint16_t* Y, int ldy,
                                        float beta, float* outVal);
spmm_status_t spmm_csrmm_heads_host_f16(int m, int d, int k, int nnz, int heads, float alpha,
                                        const int* csrRowPtr, const int* csrColInd,
                                        const float* csrVal, spmm_index_base_t base,
                                        const uint16_t* B, int ldb, float beta, float* C, int ldc);
spmm_status_t spmm_csrmm_heads_host_bf16(int m, int d, int k, int nnz, int heads, float alpha,
                                         const int* csrRowPtr, const int* csrColInd,
                                         const float* csrVal, spmm_index_base_t base,
                                         const uint16_t* B, int ldb, float beta, float* C,
                                         int ldc);
spmm_status_t spmm_csrmm_heads_f16(spmm_handle_t handle, int m, int d, int k, int nnz, int heads,
                                   float alpha, const int* csrRowPtr, const int* csrColInd,
                                   const float* csrVal, spmm_index_base_t base, const uint16_t* B,
                                   int ldb, float beta, float* C, int ldc);
spmm_status_t spmm_csrmm_heads_bf16(spmm_handle_t handle, int m, int d, int k, int nnz, int heads,
                                    float alpha, const int* csrRowPtr, const int* csrColInd,
                                    const float* csrVal, spmm_index_base_t base, const uint16_t* B,
                                    int ldb, float beta, float* C, int ldc);

/* The max / min reducers of the CSR product with the winning positions, and their backward
 * (no reference counterpart; csrc/reduce_kernels.hip): DGL's copy_u_max /
 * u_mul_e_max, PyG's aggr = "max", torch.sparse.mm(A, B, reduce = "amax" | "amin"). A is
 * m x k CSR, B [k, ldb], C [m, ldc], arg int [m, ldarg], all row-major; fp32.
 * Forward, row i with the array positions [a, b), column j < n:
 *   the term t_p = csrVal[p] * B[col(p), j]: one fp32 multiply, round to nearest, fused with
 *     nothing, subnormals kept; with csrVal == NULL (the unweighted aggregation) t_p is
 *     B[col(p), j] as stored;
 *   the winner w for SPMM_REDUCE_MAX: the lowest p whose t_p is a NaN if there is one,
 *     otherwise the lowest p with t_p >= t_q for every q under the IEEE comparison (+0 and
 *     -0 tie, and the lower position wins); SPMM_REDUCE_MIN: the same with <=;
 *   C[i, j] = t_w, the winner's own bits (the sign of a zero is the winner's; of a NaN only
 *     NaN-ness is specified); arg[i, j] = w, a 0-based position into csrColInd / csrVal
 *     whatever the index base; an empty row gives C = +0 and arg = -1.
 *   C and arg are overwritten (no alpha, no beta). arg may be NULL (inference): it is then
 *     neither computed nor written, and ldarg is not looked at.
 *   Ordered by (is-NaN, value, -position) the combine is a commutative monoid: any
 *     partition of a row over lanes, waves and workgroups gives the same C and arg, so the
 *     bits depend on the row alone, not on the grid, ld, alignment or vector width.
 * Backward: dB [k, lddb] from dC [m, lddc] and arg, over the CSR arrays of A^T (tRowPtr,
 *   tColInd: k rows) and perm (perm[q] = the position in A of transposed position q:
 *   spmm_csr2csc's perm); csrVal is in A's order, or NULL. Row c of A^T with the positions
 *   [ta, tb), L = tb - ta, column j: walk q in order, i = tColInd[q] - base,
 *   sel = (arg[i, j] == perm[q]), v = csrVal[perm[q]] (1.0f when NULL), and
 *   acc = sel ? fma(v, dC[i, j], acc) : acc, associated by the product's piece rule
 *   counted over all L positions, selected or not: pieces of max(128, ceil(L / 64))
 *   positions from the row's start, each a chain from +0, the pieces added left to right
 *   from -0; dB[c, j] is that sum (overwritten), +0 for an empty row, at every n. An
 *   unselected position contributes nothing, even where v or dC is infinite or a NaN.
 *   arg is only compared, never used as an index: a corrupt arg cannot make the entry read
 *   out of bounds. With every position selected the result is spmm_csrmm_heads_host_f32
 *   (heads = 1, alpha = 1, beta = 0) on the transposed arrays with the values
 *   csrVal[perm], bit for bit. No float atomics anywhere.
 * Checks, in spmm_csrmm_ex_f32's order: a NULL handle is SPMM_STATUS_NOT_INITIALIZED; a
 *   negative size, an op or base that is not one of the enumerators: INVALID_VALUE; m == 0
 *   or n == 0 (backward: k == 0 or n == 0) returns SUCCESS; then a NULL csrRowPtr or C, a
 *   NULL B with k > 0, a NULL csrColInd with nnz > 0 (backward: a NULL tRowPtr or dB; with
 *   nnz > 0 a NULL tColInd, perm, dC or arg), and ldb, ldc, ldarg (with arg), lddc or lddb
 *   below n: INVALID_VALUE. nnz == 0 is no quick return: C is filled with +0 and arg with
 *   -1, dB with +0. More than 65535 column tiles (n above 65535 * 64 at the narrowest
 *   lane): SPMM_STATUS_NOT_SUPPORTED.
 * The _host_ forms take host pointers and no handle and state the rules in executable form
 *   (worker threads like the other host forms); they also refuse a decreasing row pointer,
 *   a first entry below the base, a last entry - base above nnz, a column outside [0, k)
 *   (backward: outside [0, m)) and a perm entry outside [0, nnz). The device forms equal
 *   them bit for bit (tests/test_gpu_reduce.py); they do not validate (positions are
 *   clamped to [0, nnz], rows to the row count, perm to [0, nnz) where it indexes csrVal).
 * Graphs: each device entry is one kernel on the handle's stream, takes nothing from the
 *   handle's buffers (no workspace, no tickets, no keys to initialise), does not
 *   synchronise or read back, and may be captured. Every element offset of B, C, arg, dC
 *   and dB is computed in 64 bits. spmm_set_csr_waves_per_cu sizes the grids; no grid
 *   changes a bit. A row of more than 128 positions is done by the one workgroup that
 *   owns it.
 * Not served: the gradient of csrVal, half features, [nnz, heads] values,
 *   column-major operands, BSR, several GPUs. */
typedef enum { SPMM_REDUCE_MAX = 0, SPMM_REDUCE_MIN = 1 } spmm_reduce_t;
spmm_status_t spmm_csrmm_reduce_host_f32(spmm_reduce_t op, int m, int n, int k, int nnz,
                                         const int* csrRowPtr, const int* csrColInd,
                                         const float* csrVal, spmm_index_base_t base,
                                         const float* B, int ldb, float* C, int ldc, int* arg,
                                         int ldarg);
spmm_status_t spmm_csrmm_reduce_f32(spmm_handle_t handle, spmm_reduce_t op, int m, int n, int k,
                                    int nnz, const int* csrRowPtr, const int* csrColInd,
                                    const float* csrVal, spmm_index_base_t base, const float* B,
                                    int ldb, float* C, int ldc, int* arg, int ldarg);
spmm_status_t spmm_csrmm_reduce_bwd_host_f32(int k, int n, int m, int nnz, const int* tRowPtr,
                                             const int* tColInd, const int* perm,
                                             const float* csrVal, spmm_index_base_t base,
                                             const float* dC, int lddc, const int* arg,
                                             int ldarg, float* dB, int lddb);
spmm_status_t spmm_csrmm_reduce_bwd_f32(spmm_handle_t handle, int k, int n, int m, int nnz,
                                        const int* tRowPtr, const int* tColInd, const int* perm,
                                        const float* csrVal, spmm_index_base_t base,
                                        const float* dC, int lddc, const int* arg, int ldarg,
                                        float* dB, int lddb);

/* cusparseXcoo2csr (csrmm.cu:148-149): csrRowPtr[m+1] of a COO whose row
 * indices cooRowInd[nnz] are sorted ascending (device pointers, handle's
 * stream). Row indices and the output are in idxBase, as in cuSPARSE:
 * csrRowPtr[0] = idxBase, csrRowPtr[m] = nnz + idxBase. */
spmm_status_t spmm_xcoo2csr(spmm_handle_t handle, const int* cooRowInd, int nnz, int m,
                            int* csrRowPtr, spmm_index_base_t idxBase);

/* Threshold planner for divide (the reference takes `density` from the user,
 * divide.cu:348): from the histogram of block fills it picks the count
 * threshold T minimising a bytes-over-bandwidth model of the hybrid SpMM,
 *   sum_{blocks, fill >= T} (s*(bs^2 + bs*K) + 4) / bsrBytesPerSec
 * + sum_{blocks, fill <  T} fill * (8 + 4*K)    / csrBytesPerSec,
 * s = valueBytes of the BSR part, and returns density = T / bs^2 (the value
 * spmm_divide_nnz admits exactly those blocks for; T = bs^2 + 1 means "all
 * CSR"). Bandwidths <= 0 take the defaults measured on MI355X with this
 * library (BSR 7.0e12, CSR 7.5e12 algorithmic bytes/s).
 * nnzb / csrNnz / estSeconds: the split and modelled time (may be NULL). */
spmm_status_t spmm_hybrid_plan(int n, const int* rowPtr, const int* colInd, int blockDim, int K,
                               int valueBytes, double bsrBytesPerSec, double csrBytesPerSec,
                               float* density, int64_t* nnzb, int64_t* csrNnz,
                               double* estSeconds);

/* ------------------------------------------------------------------------ */
/* fp64 (T = double in gespmm_csrmm<T> / rocsparse_bsrmm_template<T>,          */
/* gespmm_csrmm.h:422, rocsparse_bsrmm.h:102): same semantics and checks as    */
/* the fp32 entry points, VALU fp64 kernels (one sequential FMA chain per CSR  */
/* output element in CSR order).                                              */
/* ------------------------------------------------------------------------ */
spmm_status_t spmm_gespmm_csrmm_f64(int A_nrows, int B_ncols, const int* A_rowPtr,
                                    const int* A_colInd, const double* A_val, const double* B,
                                    double* C, void* stream);
spmm_status_t spmm_csrmm_ex_f64(spmm_handle_t handle, int m, int n, int k, int nnz, double alpha,
                                const int* csrRowPtr, const int* csrColInd, const double* csrVal,
                                spmm_index_base_t base, const double* B, int ldb,
                                spmm_order_t orderB, double beta, double* C, int ldc,
                                spmm_order_t orderC);
/* cusparseDcsrmm2 (transA = NON_TRANSPOSE only; A^T: spmm_csr2csc_dev with valueBytes 8) */
spmm_status_t spmm_dcsrmm2(spmm_handle_t handle, spmm_operation_t transA,
                           spmm_operation_t transB, int m, int n, int k, int nnz,
                           const double* alpha, const spmm_mat_descr_t descrA,
                           const double* csrValA, const int* csrRowPtrA, const int* csrColIndA,
                           const double* B, int ldb, const double* beta, double* C, int ldc);
spmm_status_t spmm_bsrmm_ex_f64(spmm_handle_t handle, spmm_direction_t dir, int mb, int kb, int n,
                                int nnzb, int blockDim, double alpha, const int* bsrRowPtr,
                                const int* bsrColInd, const double* bsrVal, const double* B,
                                int ldb, spmm_order_t orderB, double beta, double* C, int ldc,
                                spmm_order_t orderC);
/* cusparseDbsrmm / rocsparse_bsrmm_template<double> (transA = NON_TRANSPOSE only; for A^T
 * transpose the CSR form with spmm_csr2csc_dev before it is blocked) */
spmm_status_t spmm_dbsrmm(spmm_handle_t handle, spmm_direction_t dir, spmm_operation_t transA,
                          spmm_operation_t transB, int mb, int n, int kb, int nnzb,
                          const double* alpha, const spmm_mat_descr_t descrA,
                          const double* bsrValA, const int* bsrRowPtrA, const int* bsrColIndA,
                          int blockDim, const double* B, int ldb, const double* beta, double* C,
                          int ldc);

/* ------------------------------------------------------------------------ */
/* Hybrid dense-block + CSR-remainder SpMM (divide.cu:348-373)                */
/* ------------------------------------------------------------------------ */

/* Hybrid options (per handle). At bs = 32 the hybrid runs either fused, in
 * one launch (MFMA part, then each block row's CSR remainder in the same
 * workgroup), or as two stream-ordered launches (BSR kernel, then the CSR
 * kernel with beta = 1). Same result up to the CSR kernel's split-row carries.
 * By default (flags 0) it is fused when the remainder averages at most 4096
 * entries per block row (csrNnz <= 4096 * mb); longer per-block-row
 * remainders keep the merge-path CSR kernel's balance. SPMM_HYBRID_FUSED / SPMM_HYBRID_TWO_LAUNCH force
 * one form. */
#define SPMM_HYBRID_FUSED 1
#define SPMM_HYBRID_TWO_LAUNCH 2
/* Opt-in: the bs = 32 dense-block part computes each fp32 product as six
 * bf16 MFMA products of an exact three-way bf16 split of A and B (dropped
 * terms < 2^-21 |a||b| per product; accumulation in fp32). DESIGN.md §4a.
 * Inf and NaN inputs pass through the high part (the lower parts are zeroed),
 * so non-finite values propagate as in the fp32 path. The flag takes effect
 * only on the bs = 32 LDS-staged forms: the fused launch, and the two-launch
 * BSR part when n % 4 == 0, ldb % 4 == 0 and B / bsrVal are 16-byte aligned;
 * elsewhere (bs != 32, other layouts) the
 * dense-block part runs the plain fp32 MFMA kernel, with the same result
 * within the fp32 bar. */
#define SPMM_HYBRID_SPLIT_BF16 4
spmm_status_t spmm_set_hybrid_options(spmm_handle_t handle, int flags);

/* C(m x n) = alpha * (A_bsr + A_csr) * B(k x n) + beta * C, row-major B and C.
 * A_bsr is the BSR part of spmm_sdivide (bs x bs blocks, mb = ceil(m/bs)
 * block rows), A_csr the remainder. When nnzb > 0, B must hold
 * ceil(k/bs)*bs rows and C ceil(m/bs)*bs rows (padded, as the reference's
 * drivers allocate them, run_bsrmm.cu:86-94). The BSR part runs on MFMA
 * (writing C with beta), then the CSR part accumulates (beta = 1): the result
 * is the sum of two rounded products, fma(1, fma(beta, C, alpha * S_bsr),
 * alpha * S_csr), fused launch or not. Where the two parts cancel exactly it
 * is +0; one sum over both parts would give alpha * (+0), a -0 under a
 * negative alpha (tests/test_gpu_edge_values.py::test_hybrid_csrmm_f32). */
spmm_status_t spmm_hybrid_csrmm_f32(spmm_handle_t handle, int m, int n, int k, float alpha,
                                    const int* csrRowPtr, const int* csrColInd,
                                    const float* csrVal, int csrNnz, int blockDim,
                                    const int* bsrRowPtr, const int* bsrColInd,
                                    const float* bsrVal, int nnzb, const float* B, int ldb,
                                    float beta, float* C, int ldc);

/* The same with explicit storage orders: divide.cu's own call shape
 * (divide.cu:218-230, 348-373) is csrmm2 + bsrmm onto a column-major z
 * (ldc = nb*bs) with alpha = beta = 1, B column-major (transB = N, ldb >= k)
 * or row-major (transB = T, ldb >= n). Row-major B and C are
 * spmm_hybrid_csrmm_f32. Otherwise two stream-ordered launches: a
 * column-major B is transposed once into a staging buffer of the handle's
 * that no kernel of the call writes (zero rows past k, so ldb need only cover
 * the k real rows; a row-major B must hold ceil(k/bs)*bs rows when nnzb > 0,
 * as for spmm_hybrid_csrmm_f32), the BSR part writes C in orderC with beta,
 * then the CSR remainder accumulates. A column-major C needs
 * ldc >= ceil(m/bs)*bs when nnzb > 0 (>= m otherwise). */
spmm_status_t spmm_hybrid_csrmm_ex_f32(spmm_handle_t handle, int m, int n, int k, float alpha,
                                       const int* csrRowPtr, const int* csrColInd,
                                       const float* csrVal, int csrNnz, int blockDim,
                                       const int* bsrRowPtr, const int* bsrColInd,
                                       const float* bsrVal, int nnzb, const float* B, int ldb,
                                       spmm_order_t orderB, float beta, float* C, int ldc,
                                       spmm_order_t orderC);

#ifdef __cplusplus
} /* extern "C" */
#endif

#endif /* SPMM_HIP_H */
