// transpose_kernels.hip — CSR -> CSC on the device (spmm_csr2csc_dev): the CSC form of A
// is the CSR form of A^T, so a transposed product is an ordinary product on its output.
// No reference counterpart (the reference never transposes A).
//
// The output order is the stable sort of the CSR positions by column, so every output
// byte is a function of the input alone. It is built without any per-column work, so a
// hub column costs what its entries cost anywhere else:
//   1. col_count_kernel: integer-atomic histogram of the columns into a zeroed count[n]
//      (a count does not depend on arrival order), and the validation of the columns,
//      the row pointer and nnz. A scan (scan_kernel of convert_kernels.hip, over
//      chunk sums when the array is long) turns it into cscColPtr. The host reads the flag and the total back here and gives up on a
//      bad input before anything is sorted.
//   2. ceil(bits(n - 1) / 8) passes of a stable LSD radix sort of (column, position) on
//      8-bit digits. Per pass: digit_count_kernel (a workgroup owns a tile of kTile
//      consecutive elements and counts its digits in LDS), one scan of the (digit, tile)
//      counts in digit-major order, digit_scatter_kernel (each wave walks its contiguous
//      share of the tile in 64-element steps; a lane finds the lanes of its step with
//      the same digit by eight ballots and ranks itself among them by a popcount of the
//      lower lanes, on top of the wave's running per-digit offset in LDS, which starts
//      at the tile's scanned offset plus the counts of the waves before it). The LDS
//      integer atomics only count; nothing whose arrival order could reach the output
//      goes through an atomic. The first pass reads csrColInd itself with the position
//      implied, the last writes positions only (into perm when the caller wants it).
//   3. expand_rows_kernel writes the row of every position once, and csc_gather_kernel
//      reads the row and the value bits (2 / 4 / 8-byte words) of each sorted position.
//      The alternative, a binary search of csrRowPtr inside the gather, needs 4 bytes
//      per nonzero less and measured slower on every workload.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cstdint>

#include "context.hpp"
#include "launch_record.hpp"

namespace {

constexpr int kWave = 64;
constexpr int kWG = 256;
constexpr int kSortWG = 512;
constexpr int kSortWaves = kSortWG / kWave;
constexpr int kSteps = 16;                       // 64-element steps per wave
constexpr int kWaveShare = kSteps * kWave;       // consecutive elements of one wave
constexpr int kTile = kSortWaves * kWaveShare;   // 8192 elements per workgroup
constexpr int kDigits = 256;

__global__ __launch_bounds__(kWG) void fill_int_kernel(int* __restrict__ out, long long count,
                                                       int value) {
  for (long long i = (long long)blockIdx.x * kWG + threadIdx.x; i < count;
       i += (long long)gridDim.x * kWG)
    out[i] = value;
}

// First position of the matrix in colind / val (views: csrRowPtr[0] may exceed the base).
__device__ __forceinline__ long long first_pos(const int* rowptr, int baseA) {
  return (long long)rowptr[0] - baseA;
}

// count[c] = entries of column c; *bad = 1 on a column outside [0, n) (skipped, never
// used as an index), a decreasing row pointer, a first position below 0 or an nnz other
// than csrRowPtr[m] - csrRowPtr[0].
__global__ __launch_bounds__(kWG) void col_count_kernel(int m, int n, int nnz,
                                                        const int* __restrict__ rowptr,
                                                        const int* __restrict__ colind,
                                                        int baseA, int* __restrict__ count,
                                                        int* __restrict__ bad) {
  const long long p0 = first_pos(rowptr, baseA);
  const long long tid = (long long)blockIdx.x * kWG + threadIdx.x;
  const long long stride = (long long)gridDim.x * kWG;
  int flag = 0;
  if (tid == 0 && (p0 < 0 || (long long)rowptr[m] - rowptr[0] != nnz)) flag = 1;
  for (long long r = tid; r < m; r += stride)
    if (rowptr[r + 1] < rowptr[r]) flag = 1;
  if (p0 >= 0)
    for (long long i = tid; i < nnz; i += stride) {
      const int c = colind[p0 + i] - baseA;
      if (c >= 0 && c < n) atomicAdd(&count[c], 1);
      else flag = 1;
    }
  if (flag) *bad = 1;
}

// Exclusive scan of a long count array in three launches (the one-workgroup scan_kernel
// of convert_kernels.hip walks 16 K counts per step: 1.7 ms on the 1.9 M tile counts of
// the products stand-in, more than the scatter they serve): the sum of every chunk of
// kChunk counts, scan_kernel over those sums, then every chunk scanned from its offset.
// Integer sums: the grouping cannot change a bit.
constexpr int kScanPer = 16;
constexpr int kChunk = kWG * kScanPer;  // counts per workgroup

__global__ __launch_bounds__(kWG) void chunk_sum_kernel(const int* __restrict__ count, int len,
                                                        int* __restrict__ sums) {
  __shared__ int part[kWG / kWave];
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wv = tid >> 6;
  const long long i0 = (long long)blockIdx.x * kChunk + (long long)tid * kScanPer;
  int s = 0;
#pragma unroll
  for (int k = 0; k < kScanPer; ++k)
    if (i0 + k < len) s += count[i0 + k];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
  if (lane == 0) part[wv] = s;
  __syncthreads();
  if (tid == 0) {
    int t = 0;
#pragma unroll
    for (int w = 0; w < kWG / kWave; ++w) t += part[w];
    sums[blockIdx.x] = t;
  }
}

// out[i + 1] = base + count[0] + ... + count[i]; chunk_off[b] = counts before chunk b.
__global__ __launch_bounds__(kWG) void chunk_scan_kernel(const int* __restrict__ count, int len,
                                                         const int* __restrict__ chunk_off,
                                                         int base, int* __restrict__ out) {
  __shared__ int part[kWG / kWave];
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wv = tid >> 6;
  const long long i0 = (long long)blockIdx.x * kChunk + (long long)tid * kScanPer;
  int v[kScanPer], s = 0;
#pragma unroll
  for (int k = 0; k < kScanPer; ++k) {
    v[k] = i0 + k < len ? count[i0 + k] : 0;
    s += v[k];
  }
  int x = s;  // inclusive wave scan of the threads' sums
#pragma unroll
  for (int o = 1; o < kWave; o <<= 1) {
    const int y = __shfl_up(x, o);
    if (lane >= o) x += y;
  }
  if (lane == kWave - 1) part[wv] = x;
  __syncthreads();
  int run = chunk_off[blockIdx.x] + base + x - s;
  for (int w = 0; w < wv; ++w) run += part[w];
#pragma unroll
  for (int k = 0; k < kScanPer; ++k) {
    run += v[k];
    if (i0 + k < len) out[i0 + k + 1] = run;
  }
  if (blockIdx.x == 0 && tid == 0) out[0] = base;
}

// rows[i] = row of the matrix's i-th position. A wave takes eight rows at a time, eight
// lanes per row for a row's first 64 entries; what a longer row has beyond them is
// written by the whole wave, one such row after the other (a hub row of 13 K entries
// would otherwise keep eight lanes busy for 1.6 K steps). Every index is clamped to
// [0, nnz] first, so no row pointer can lead a store outside rows[0 .. nnz).
__global__ __launch_bounds__(kWG) void expand_rows_kernel(int m, int nnz,
                                                          const int* __restrict__ rowptr,
                                                          int* __restrict__ rows) {
  const int lane = threadIdx.x & (kWave - 1), sub = lane & 7, grp = lane >> 3;
  const long long wave = ((long long)blockIdx.x * kWG + threadIdx.x) >> 6;
  const long long nwaves = ((long long)gridDim.x * kWG) >> 6;
  const long long first = rowptr[0];
  for (long long r0 = wave * 8; r0 < m; r0 += nwaves * 8) {  // wave-uniform
    const long long r = r0 + grp;
    int a = 0, b = 0;
    if (r < m) {
      a = (int)std::min<long long>(std::max<long long>(rowptr[r] - first, 0), nnz);
      b = (int)std::min<long long>(std::max<long long>(rowptr[r + 1] - first, 0), nnz);
    }
    const int head = b - a > kWave ? a + kWave : b;
    for (long long i = (long long)a + sub; i < head; i += 8) rows[i] = (int)r;
    unsigned long long more = __ballot(b - a > kWave);
    while (more) {
      const int src = __ffsll((long long)more) - 1;  // first lane of the row's group
      more &= ~(0xffull << src);
      const int ra = __shfl(a, src), rb = __shfl(b, src);
      const int rr = (int)(r0 + (src >> 3));
      for (long long i = (long long)ra + kWave + lane; i < rb; i += kWave) rows[i] = rr;
    }
  }
}

__device__ __forceinline__ int digit_of(int key, int shift) {
  return (int)(((unsigned)key >> shift) & (kDigits - 1));
}

// tile_count[d * ntiles + tile] = elements of the tile whose digit is d. FIRST: the keys
// are csrColInd's own (from the first position on, minus the base).
template <bool FIRST>
__global__ __launch_bounds__(kSortWG) void digit_count_kernel(int nnz, int ntiles, int shift,
                                                              const int* __restrict__ keys,
                                                              const int* __restrict__ rowptr,
                                                              int baseA,
                                                              int* __restrict__ tile_count) {
  __shared__ int hist[kDigits];
  const int tid = threadIdx.x, tile = blockIdx.x;
  if (tid < kDigits) hist[tid] = 0;
  __syncthreads();
  const long long p0 = FIRST ? std::max<long long>(first_pos(rowptr, baseA), 0) : 0;
  const int sub = FIRST ? baseA : 0;
  const long long t0 = (long long)tile * kTile;
  for (int e = tid; e < kTile; e += kSortWG) {
    const long long i = t0 + e;
    if (i < nnz) atomicAdd(&hist[digit_of(keys[p0 + i] - sub, shift)], 1);
  }
  __syncthreads();
  if (tid < kDigits) tile_count[(size_t)tid * ntiles + tile] = hist[tid];
}

// Element i of the tile goes to prefix[digit][tile] + (elements of the tile before i with
// the same digit). LAST: only the positions are written.
template <bool FIRST, bool LAST>
__global__ __launch_bounds__(kSortWG) void digit_scatter_kernel(
    int nnz, int ntiles, int shift, const int* __restrict__ keys_in,
    const int* __restrict__ pay_in, const int* __restrict__ rowptr, int baseA,
    const int* __restrict__ prefix, int* __restrict__ keys_out, int* __restrict__ pay_out) {
  // per wave and digit: first the wave's count, then its running output offset
  __shared__ int woff[kSortWaves][kDigits];
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wv = tid >> 6, tile = blockIdx.x;
  for (int i = tid; i < kSortWaves * kDigits; i += kSortWG) (&woff[0][0])[i] = 0;
  __syncthreads();
  const long long p0 = FIRST ? std::max<long long>(first_pos(rowptr, baseA), 0) : 0;
  const long long w0 = (long long)tile * kTile + (long long)wv * kWaveShare;
  int key[kSteps], pay[kSteps];
#pragma unroll
  for (int s = 0; s < kSteps; ++s) {
    const long long i = w0 + s * kWave + lane;
    key[s] = 0;
    pay[s] = 0;
    if (i < nnz) {
      key[s] = FIRST ? keys_in[p0 + i] - baseA : keys_in[i];
      pay[s] = FIRST ? (int)(p0 + i) : pay_in[i];
      atomicAdd(&woff[wv][digit_of(key[s], shift)], 1);
    }
  }
  __syncthreads();
  if (tid < kDigits) {  // the waves' counts, combined in wave order
    int run = prefix[(size_t)tid * ntiles + tile];
#pragma unroll
    for (int w = 0; w < kSortWaves; ++w) {
      const int c = woff[w][tid];
      woff[w][tid] = run;
      run += c;
    }
  }
  __syncthreads();
  volatile int* mine = woff[wv];
  const unsigned long long below = (1ull << lane) - 1ull;
#pragma unroll
  for (int s = 0; s < kSteps; ++s) {
    const bool valid = w0 + s * kWave + lane < nnz;
    const int d = digit_of(key[s], shift);
    unsigned long long peers = __ballot(valid);
#pragma unroll
    for (int b = 0; b < 8; ++b) {
      const bool bit = (d >> b) & 1;
      const unsigned long long has = __ballot(valid && bit);
      peers &= bit ? has : ~has;
    }
    const int rank = __popcll(peers & below);
    int base = 0;
    if (valid) base = mine[d];
    __builtin_amdgcn_wave_barrier();
    if (valid && rank == 0) mine[d] = base + __popcll(peers);
    __builtin_amdgcn_wave_barrier();
    const int dst = base + rank;
    if (valid && dst >= 0 && dst < nnz) {
      if (!LAST) keys_out[dst] = key[s];
      pay_out[dst] = pay[s];
    }
  }
}

// Entry i of the output: its position p (pos[i], or the i-th position when nothing was
// sorted), its row (rows[] by the position's index in the matrix) and its VB value bytes.
template <int VB>
__global__ __launch_bounds__(kWG) void csc_gather_kernel(int nnz,
                                                         const int* __restrict__ rowptr,
                                                         int baseA, int baseC,
                                                         const int* pos,
                                                         const int* __restrict__ rows,
                                                         const void* __restrict__ val,
                                                         int* __restrict__ rowind,
                                                         void* __restrict__ cscval, int* perm) {
  const long long p0 = std::max<long long>(first_pos(rowptr, baseA), 0);
  for (long long i = (long long)blockIdx.x * kWG + threadIdx.x; i < nnz;
       i += (long long)gridDim.x * kWG) {
    const long long p = pos ? (long long)pos[i] : p0 + i;
    if (p < p0 || p >= p0 + nnz) continue;  // never taken on a sorted valid input
    rowind[i] = rows[p - p0] + baseC;
    if (perm && perm != pos) perm[i] = (int)p;
    if constexpr (VB == 2) static_cast<uint16_t*>(cscval)[i] = static_cast<const uint16_t*>(val)[p];
    if constexpr (VB == 4) static_cast<uint32_t*>(cscval)[i] = static_cast<const uint32_t*>(val)[p];
    if constexpr (VB == 8) static_cast<uint64_t*>(cscval)[i] = static_cast<const uint64_t*>(val)[p];
  }
}

inline size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

inline unsigned grid_for(long long count) {
  return (unsigned)std::min<long long>(std::max<long long>((count + kWG - 1) / kWG, 1), 65536);
}

// Radix passes for keys in [0, n): ceil(bits(n - 1) / 8).
inline int radix_passes(int n) {
  if (n <= 1) return 0;
  const int bits = 32 - __builtin_clz((unsigned)(n - 1));
  return (bits + 7) / 8;
}

// One kernel of the conversion (or the launches of one scan), between a timing pair when
// the handle times kernels.
template <typename F>
inline void timed(spmm_context* ctx, F launch) {
  const int slot = spmm::timing_begin(ctx);
  launch();
  spmm::timing_end(ctx, slot);
}

inline int scan_chunks(size_t len) { return (int)((len + kChunk - 1) / kChunk); }

// out[0 .. len] = base + the exclusive scan of count[0 .. len), *total = the sum. Up to
// one chunk: scan_kernel alone; longer: chunk sums, their scan, the chunks (sums: one
// int per chunk, offs: one more).
inline void scan_counts(spmm_context* ctx, const int* count, int len, int* out, long long* total,
                        int base, int* sums, int* offs) {
  if (len <= kChunk) {
    (void)spmm::launch_scan_counts(ctx, count, len, out, total, base);
    return;
  }
  const int nb = scan_chunks((size_t)len);
  SPMM_LAUNCH(ctx, chunk_sum_kernel, dim3(nb), dim3(kWG), 0, count, len, sums);
  (void)spmm::launch_scan_counts(ctx, sums, nb, offs, total, 0);
  SPMM_LAUNCH(ctx, chunk_scan_kernel, dim3(nb), dim3(kWG), 0, count, len, offs,
              base, out);
}

}  // namespace

extern "C" {

spmm_status_t spmm_csr2csc_dev(spmm_handle_t handle, int m, int n, int nnz,
                               const spmm_mat_descr_t descrA, const void* csrVal,
                               const int* csrRowPtr, const int* csrColInd, int valueBytes,
                               const spmm_mat_descr_t descrC, void* cscVal, int* cscColPtr,
                               int* cscRowInd, int* perm) {
  if (!handle) return SPMM_STATUS_NOT_INITIALIZED;
  if (!descrA || !descrC || m < 0 || n < 0 || nnz < 0) return SPMM_STATUS_INVALID_VALUE;
  if (valueBytes != 0 && valueBytes != 2 && valueBytes != 4 && valueBytes != 8)
    return SPMM_STATUS_INVALID_VALUE;
  if (!csrRowPtr || !cscColPtr) return SPMM_STATUS_INVALID_VALUE;
  if (nnz > 0 && (!csrColInd || !cscRowInd || (valueBytes > 0 && (!csrVal || !cscVal))))
    return SPMM_STATUS_INVALID_VALUE;
  if (nnz > 0 && n == 0) return SPMM_STATUS_INVALID_VALUE;  // every column is out of range
  spmm_context* ctx = handle;
  // The call reads a flag back and synchronises for it: refused under capture before
  // anything is queued.
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(ctx->stream, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone)
    return SPMM_STATUS_NOT_SUPPORTED;
  const int baseA = (int)descrA->base, baseC = (int)descrC->base;
  if (nnz == 0) {
    SPMM_LAUNCH(ctx, fill_int_kernel, dim3(grid_for((long long)n + 1)), dim3(kWG), 0, cscColPtr,
                (long long)n + 1, baseC);
    return spmm::from_hip(hipGetLastError());
  }
  const int passes = radix_passes(n);
  const int ntiles = (int)(((long long)nnz + kTile - 1) / kTile);
  const size_t ncount = (size_t)kDigits * ntiles;
  const int nkeys = std::min(std::max(passes - 1, 0), 2);
  const int npay = std::min(perm ? std::max(passes - 1, 0) : passes, 2);
  // header (total, flag) | count[n] | tile counts | their scan | the scans' chunk sums and
  // offsets | key and position buffers | the rows of the positions
  const size_t nchunks = (size_t)scan_chunks(std::max((size_t)n, ncount)) + 1;
  const size_t off_count = 256;
  const size_t off_tc = off_count + align256(sizeof(int) * (size_t)n);
  const size_t off_pf = off_tc + align256(sizeof(int) * ncount);
  const size_t off_cs = off_pf + align256(sizeof(int) * (ncount + 1));
  const size_t off_buf = off_cs + 2 * align256(sizeof(int) * nchunks);
  const size_t buf_bytes = align256(sizeof(int) * (size_t)nnz);
  const size_t need = off_buf + buf_bytes * (size_t)(nkeys + npay + 1);
  if (spmm_status_t st = spmm::ensure_workspace(ctx, need); st != SPMM_STATUS_SUCCESS) return st;
  char* ws = static_cast<char*>(ctx->ws);
  long long* total = reinterpret_cast<long long*>(ws);
  int* bad = reinterpret_cast<int*>(ws + 8);
  int* count = reinterpret_cast<int*>(ws + off_count);
  int* tile_count = reinterpret_cast<int*>(ws + off_tc);
  int* prefix = reinterpret_cast<int*>(ws + off_pf);
  int* sums = reinterpret_cast<int*>(ws + off_cs);
  int* offs = reinterpret_cast<int*>(ws + off_cs + align256(sizeof(int) * nchunks));
  int* kbuf[2] = {reinterpret_cast<int*>(ws + off_buf),
                  reinterpret_cast<int*>(ws + off_buf + buf_bytes)};
  int* pbuf[2] = {reinterpret_cast<int*>(ws + off_buf + buf_bytes * nkeys),
                  reinterpret_cast<int*>(ws + off_buf + buf_bytes * (nkeys + 1))};

  if (hipMemsetAsync(ws, 0, off_count + sizeof(int) * (size_t)n, ctx->stream) != hipSuccess)
    return SPMM_STATUS_EXECUTION_FAILED;
  timed(ctx, [&] {
    SPMM_LAUNCH(ctx, col_count_kernel, dim3(grid_for(std::max<long long>(nnz, m))), dim3(kWG),
                0, m, n, nnz, csrRowPtr, csrColInd, baseA, count, bad);
  });
  timed(ctx, [&] { scan_counts(ctx, count, n, cscColPtr, total, baseC, sums, offs); });
  long long host[2] = {0, 0};
  if (hipMemcpyAsync(host, ws, 16, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess ||
      hipStreamSynchronize(ctx->stream) != hipSuccess)
    return SPMM_STATUS_EXECUTION_FAILED;
  if ((int)(host[1] & 0xffffffff) != 0 || host[0] != nnz) return SPMM_STATUS_INVALID_VALUE;

  const int* keys_in = csrColInd;
  const int* pay_in = nullptr;
  const int* sorted = nullptr;  // stays null when there is nothing to sort (n <= 1)
  for (int j = 0; j < passes; ++j) {
    const bool first = j == 0, last = j == passes - 1;
    const int shift = 8 * j;
    int* keys_out = last ? nullptr : kbuf[j & 1];
    int* pay_out = last && perm ? perm : pbuf[j & 1];
    timed(ctx, [&] {
      if (first)
        SPMM_LAUNCH(ctx, digit_count_kernel<true>, dim3(ntiles), dim3(kSortWG), 0,
                    nnz, ntiles, shift, keys_in, csrRowPtr, baseA, tile_count);
      else
        SPMM_LAUNCH(ctx, digit_count_kernel<false>, dim3(ntiles), dim3(kSortWG), 0,
                    nnz, ntiles, shift, keys_in, csrRowPtr, baseA, tile_count);
    });
    timed(ctx, [&] { scan_counts(ctx, tile_count, (int)ncount, prefix, total, 0, sums, offs); });
    timed(ctx, [&] {
#define SPMM_SCATTER(F, L)                                                                    \
  SPMM_LAUNCH(ctx, (digit_scatter_kernel<F, L>), dim3(ntiles), dim3(kSortWG), 0, \
              nnz, ntiles, shift, keys_in, pay_in, csrRowPtr, baseA, prefix, keys_out,   \
              pay_out)
      if (first && last) SPMM_SCATTER(true, true);
      else if (first) SPMM_SCATTER(true, false);
      else if (last) SPMM_SCATTER(false, true);
      else SPMM_SCATTER(false, false);
#undef SPMM_SCATTER
    });
    keys_in = keys_out;
    pay_in = pay_out;
    sorted = pay_out;
  }
  int* rows = reinterpret_cast<int*>(ws + off_buf + buf_bytes * (size_t)(nkeys + npay));
  timed(ctx, [&] {
    SPMM_LAUNCH(ctx, expand_rows_kernel, dim3(grid_for((long long)m * 8)), dim3(kWG), 0, m, nnz,
                csrRowPtr, rows);
  });
  timed(ctx, [&] {
    const dim3 grid(grid_for(nnz));
#define SPMM_GATHER(VB)                                                                      \
  SPMM_LAUNCH(ctx, csc_gather_kernel<VB>, grid, dim3(kWG), 0, nnz, csrRowPtr, \
              baseA, baseC, sorted, rows, csrVal, cscRowInd, cscVal, perm)
    if (valueBytes == 0) SPMM_GATHER(0);
    else if (valueBytes == 2) SPMM_GATHER(2);
    else if (valueBytes == 4) SPMM_GATHER(4);
    else SPMM_GATHER(8);
#undef SPMM_GATHER
  });
  return spmm::from_hip(hipGetLastError());
}

}  // extern "C"
