// dispatch_trace — which kernel instantiation, grid and arguments every launcher of
// csr_kernels.hip and bsr_kernels.hip reaches, over a grid of arguments, on the host alone.
//
// Links host-only objects of the two files built with -DSPMM_DISPATCH_TRACE
// (csrc/dispatch_trace.hpp turns each launch into a line) and not context.cpp: the handle
// services the launchers call are the stubs below, and num_cus is fixed at 256, so the
// output is the same on every machine. Pointers are fake (no launcher reads device memory
// on the host). tests/test_dispatch_trace.py compares stdout with
// tests/golden/dispatch_trace.txt.
//
// Output, per launcher: a header "## <launcher> calls=<n> fnv=<hash>", then each distinct
// line once with its count, grouped under its first word ("@ <tag>", then "<count> <rest of
// the line>"), tags and lines in order of first appearance. A line is a launch
// (dispatch_trace.hpp) or a call's result ("= status <s>", with the small-path record for
// the fp32 BSR entry). The hash (FNV-1a, 64 bits) is over every line of every call in call
// order, so the sequence within each call is pinned too, not only the set of lines.
//
// With the argument "cases" the program instead reads one launcher call per line of
// standard input and answers each with one line: the tags of the kernels that call
// launches, in order (tests/test_kernel_cases.py asks it which kernels the cases of
// tests/kernel_cases.py reach). The lines, all fields integers:
//   bsr f16 bs n rowd brow crow voff boff coff ldb ldc mb kb nnzb masks dense bsr_flags hybrid_flags
//   csr f16 m n boff coff ldb ldc nnz hot csr_flags
//   hybrid m n ldb ldc hybrid_flags
//
// The argument grids are subsets of the full product (which runs to millions of calls):
// the arguments that pick a kernel family (bs, direction, orders, n) are crossed in full,
// and every other argument is varied one at a time (a few in pairs) from a set of base
// cases that reaches every family. The loops below are the definition.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <map>
#include <sstream>
#include <string>
#include <vector>

#include "context.hpp"

// A host-only object still registers its (absent) device code at start-up, through an
// undefined __hip_fatbin_<id> symbol; the Makefile's link line points those here. Nothing
// in this program starts the HIP runtime, so the empty image is never parsed.
extern "C" {
extern const char spmm_trace_no_fatbin[64] = {};
}

namespace {
bool g_cases;                     // "cases" mode: emit() keeps the launches' tags only
std::vector<std::string> g_tags;
std::vector<std::string> g_order;
std::map<std::string, long> g_count;
uint64_t g_hash;
long g_calls;

void section_begin() {
  g_order.clear();
  g_count.clear();
  g_hash = 1469598103934665603ull;
  g_calls = 0;
}
void section_end(const char* name) {
  std::printf("## %s calls=%ld fnv=%016llx\n", name, g_calls, (unsigned long long)g_hash);
  // grouped by a line's first word (a launch's tag, or "="), each printed once as "@ <word>"
  std::vector<std::string> heads;
  std::map<std::string, std::vector<const std::string*>> by_head;
  for (const std::string& l : g_order) {
    std::vector<const std::string*>& v = by_head[l.substr(0, l.find(' '))];
    if (v.empty()) heads.push_back(l.substr(0, l.find(' ')));
    v.push_back(&l);
  }
  for (const std::string& h : heads) {
    std::printf("@ %s\n", h.c_str());
    for (const std::string* l : by_head[h])
      std::printf("%ld%s\n", g_count[*l], l->c_str() + h.size());
  }
}

void* grow(void** p, size_t* have, size_t need) {
  if (need > *have) {
    std::free(*p);
    *p = std::malloc(need);
    *have = *p ? need : 0;
  }
  return *p;
}
}  // namespace

namespace spmm_trace {
void emit(const std::string& line) {
  if (g_cases) {
    if (line[0] != '=') g_tags.push_back(line.substr(0, line.find(' ')));
    return;
  }
  for (unsigned char c : line) g_hash = (g_hash ^ c) * 1099511628211ull;
  g_hash = (g_hash ^ '\n') * 1099511628211ull;
  if (g_count[line]++ == 0) g_order.push_back(line);
}
}  // namespace spmm_trace

// The handle services of context.cpp, on host memory.
namespace spmm {
spmm_status_t ensure_scratch(spmm_context* ctx, size_t bytes) {
  return grow(&ctx->scratch, &ctx->scratch_bytes, bytes) ? SPMM_STATUS_SUCCESS
                                                         : SPMM_STATUS_ALLOC_FAILED;
}
spmm_status_t ensure_order_buffer(spmm_context* ctx, size_t n) {
  void* p = ctx->order;
  size_t have = ctx->order_cap * sizeof(int);
  ctx->order = static_cast<int*>(grow(&p, &have, n * sizeof(int)));
  ctx->order_cap = have / sizeof(int);
  return ctx->order ? SPMM_STATUS_SUCCESS : SPMM_STATUS_ALLOC_FAILED;
}
spmm_status_t ensure_tickets(spmm_context* ctx, size_t n) {
  void* p = ctx->tickets;
  size_t have = ctx->tickets_cap * sizeof(int);
  ctx->tickets = static_cast<int*>(grow(&p, &have, n * sizeof(int)));
  ctx->tickets_cap = have / sizeof(int);
  return ctx->tickets ? SPMM_STATUS_SUCCESS : SPMM_STATUS_ALLOC_FAILED;
}
int timing_begin(spmm_context*) { return -1; }
void timing_end(spmm_context*, int) {}
}  // namespace spmm

namespace {

spmm_context* g_ctx;

void result(spmm_status_t st, bool small = false) {
  std::string s = "= status " + std::to_string((int)st);
  if (small)
    s += " small_path " + std::to_string(g_ctx->small_path) + " bs " +
         std::to_string(g_ctx->small_path_bs);
  spmm_trace::emit(s);
  ++g_calls;
}

// fake device arrays: 256-byte aligned bases far apart, plus a byte offset
template <typename T>
T* fake(int which, int off = 0) {
  return reinterpret_cast<T*>((uintptr_t)0x100000000ull * (which + 1) + off);
}
const int* kRowptr = fake<const int>(0);
const int* kColind = fake<const int>(1);
const unsigned* kMasks = fake<const unsigned>(5);

constexpr int kNs[] = {4, 30, 64, 68, 128, 132, 256, 260};
constexpr int kBs[] = {2, 3, 4, 8, 16, 32, 64};
constexpr int kShallow = 64, kDeep = 25000;  // block rows: against 8 * 12 * num_cus waves
constexpr int kWideLdb = 1 << 24;            // ldb * 128 >= 2^31

struct BsrCase {
  int bs = 32, n = 132;
  bool rowd = true, brow = true, crow = true;
  int voff = 0, boff = 0, coff = 0;  // bytes off 16-byte alignment
  int ldb_add = 0, ldc_add = 0;      // ldb = n + ldb_add (or kWideLdb when wide)
  bool wide = false;
  int nnzb = 100, mb = kShallow, kb = 0;  // kb = 0: mb
  bool masks = false, dense = false;
  int bsr_flags = 0, hybrid_flags = 0;
};

void run_bsr(const BsrCase& c, bool f16, int ldb_abs = 0, int ldc_abs = 0) {
  g_ctx->bsr_flags = c.bsr_flags;
  g_ctx->hybrid_flags = c.hybrid_flags;
  g_ctx->small_path = -1;
  g_ctx->small_path_bs = 0;
  const auto dir = c.rowd ? SPMM_DIRECTION_ROW : SPMM_DIRECTION_COLUMN;
  const auto ob = c.brow ? SPMM_ORDER_ROW : SPMM_ORDER_COL;
  const auto oc = c.crow ? SPMM_ORDER_ROW : SPMM_ORDER_COL;
  // a column-major operand's leading dimension counts rows
  const int rows_b = (c.kb ? c.kb : c.mb) * c.bs, rows_c = c.mb * c.bs;
  const int ldb = ldb_abs ? ldb_abs : c.wide ? kWideLdb : (c.brow ? c.n : rows_b) + c.ldb_add;
  const int ldc = ldc_abs ? ldc_abs : (c.crow ? c.n : rows_c) + c.ldc_add;
  const int kb = c.kb ? c.kb : c.mb;
  float* C = fake<float>(4, c.coff);
  const unsigned* masks = c.masks ? kMasks : nullptr;
  if (f16)
    result(spmm::launch_bsrmm_f16(g_ctx, dir, c.mb, kb, c.n, c.nnzb, c.bs, 1.f, kRowptr, kColind,
                                  fake<const uint16_t>(2, c.voff), fake<const uint16_t>(3, c.boff),
                                  ldb, ob, 0.f, C, ldc, oc, masks));
  else
    result(spmm::launch_bsrmm_f32(g_ctx, dir, c.mb, kb, c.n, c.nnzb, c.bs, 1.f, kRowptr, kColind,
                                  fake<const float>(2, c.voff), fake<const float>(3, c.boff), ldb,
                                  ob, 0.f, C, ldc, oc, c.dense, masks),
           true);
}

void bsr_grid(bool f16) {
  // 1. the family-picking arguments in full: bs x direction x both orders x n (a block
  // size that only the generic kernel serves, 3 and every fp16 size but 16, at one n;
  // fp16 bs 8 stands for them at every n; column-major B, which only the fragment and
  // generic kernels read, at two n)
  for (int bs : kBs)
    for (int rowd = 1; rowd >= 0; --rowd)
      for (int brow = 1; brow >= 0; --brow)
        for (int crow = 1; crow >= 0; --crow)
          for (int n : kNs) {
            if ((bs == 3 || (f16 && bs != 16 && bs != 8)) && n != 64) continue;
            if (!brow && n != 64 && n != 132) continue;
            BsrCase c;
            c.bs = bs, c.n = n, c.rowd = rowd, c.brow = brow, c.crow = crow;
            run_bsr(c, f16);
          }
  // 2. one argument at a time (and the pairs that meet in one rule) from base cases: ROW
  // blocks on row-major B, COLUMN blocks with masks (the analysed streams), both with C in
  // either order and n on both sides of the 64-column tile (at widths both precisions'
  // streams take), and column-major B once. Only the block sizes with kernels of their own
  // that the rules tell apart: fp32 8, 16, 32, 64 (3 is always the generic kernel, 2 and
  // 4 differ from 8 by a template argument alone); fp16 16 (every other size is the
  // generic kernel whatever the layout: step 1).
  const std::vector<int> bases_bs = f16 ? std::vector<int>{16} : std::vector<int>{8, 16, 32, 64};
  for (int bs : bases_bs)
    for (int base = 0; base < 3; ++base)
      for (int crow = 1; crow >= (base == 2 ? 1 : 0); --crow)
        for (int n : {64, 256}) {
          if (base == 2 && n != 64) continue;
          BsrCase b;
          b.bs = bs, b.n = n, b.crow = crow;
          b.rowd = base != 1, b.masks = base == 1, b.brow = base != 2;
          std::vector<BsrCase> v;
          auto add = [&](auto&& f) {
            v.push_back(b);
            f(v.back());
          };
          for (int off : {4, 8}) {
            add([&](BsrCase& c) { c.voff = off; });
            add([&](BsrCase& c) { c.boff = off; });
            add([&](BsrCase& c) { c.coff = off; });
          }
          for (int a : {1, 4}) {
            add([&](BsrCase& c) { c.ldb_add = a; });
            add([&](BsrCase& c) { c.ldc_add = a; });
          }
          add([&](BsrCase& c) { c.wide = true; });
          add([&](BsrCase& c) { c.wide = true, c.masks = false; });
          add([&](BsrCase& c) { c.wide = true, c.nnzb = 1 << 15; });
          for (int nnzb : {0, 1 << 15, 1 << 20}) {
            add([&](BsrCase& c) { c.nnzb = nnzb; });
            add([&](BsrCase& c) { c.nnzb = nnzb, c.mb = kDeep; });
          }
          add([&](BsrCase& c) { c.mb = kDeep; });
          add([&](BsrCase& c) { c.masks = !c.masks; });
          add([&](BsrCase& c) { c.dense = true; });
          add([&](BsrCase& c) { c.dense = true, c.hybrid_flags = SPMM_HYBRID_SPLIT_BF16; });
          add([&](BsrCase& c) { c.hybrid_flags = SPMM_HYBRID_SPLIT_BF16; });
          add([&](BsrCase& c) { c.bsr_flags = SPMM_BSR_DENSE_BLOCK_PRODUCT; });
          add([&](BsrCase& c) {
            c.bsr_flags = SPMM_BSR_DENSE_BLOCK_PRODUCT, c.hybrid_flags = SPMM_HYBRID_SPLIT_BF16;
          });
          add([&](BsrCase& c) { c.bsr_flags = SPMM_BSR_SMALL_GROUPED; });
          add([&](BsrCase& c) {
            c.bsr_flags = SPMM_BSR_SMALL_GROUPED | SPMM_BSR_DENSE_BLOCK_PRODUCT;
          });
          // the grouped small stream's own limits, under the flag that forces it
          add([&](BsrCase& c) { c.bsr_flags = SPMM_BSR_SMALL_GROUPED, c.kb = 1 << 26; });
          add([&](BsrCase& c) { c.bsr_flags = SPMM_BSR_SMALL_GROUPED, c.coff = 8; });
          add([&](BsrCase& c) { c.bsr_flags = SPMM_BSR_SMALL_GROUPED, c.boff = 8; });
          add([&](BsrCase& c) { c.bsr_flags = SPMM_BSR_SMALL_GROUPED, c.ldb_add = 2; });
          add([&](BsrCase& c) { c.bsr_flags = SPMM_BSR_SMALL_GROUPED, c.mb = kDeep; });
          for (const BsrCase& c : v) run_bsr(c, f16);
        }
  // 3. the grouped small stream at the block sizes step 2 leaves to bs 8
  for (int bs : {2, 4})
    for (int rowd = 1; rowd >= 0; --rowd)
      for (int crow = 1; crow >= 0; --crow) {
        BsrCase c;
        c.bs = bs, c.n = 256, c.rowd = rowd, c.crow = crow, c.bsr_flags = SPMM_BSR_SMALL_GROUPED;
        run_bsr(c, f16);
      }
  // 4. empty products
  for (int z = 0; z < 2; ++z) {
    BsrCase c;
    (z ? c.mb : c.n) = 0;
    run_bsr(c, f16);
  }
}

void hybrid_grid() {
  for (int flags : {0, (int)SPMM_HYBRID_SPLIT_BF16})
    for (int m : {0, 2048, 2049, 32 * 9000})  // 4 workgroups per CU: shallow up to 8192 waves
      for (int n : {0, 4, 64, 132, 256}) {
        g_ctx->hybrid_flags = flags;
        result(spmm::launch_hybrid32_fused(g_ctx, m, n, 1.f, kRowptr, kColind,
                                           fake<const float>(2), fake<const int>(6),
                                           fake<const int>(7), fake<const float>(8),
                                           fake<const float>(3), n + 4, 0.f, fake<float>(4), n));
      }
  g_ctx->hybrid_flags = 0;
  std::string fus = "= fusable ";  // hybrid32_fusable: n, ldb, ldc, bval, B, C one bit each
  for (int i = 0; i < 64; ++i) {
    const int n = i & 1 ? 6 : 8, ldb = i & 2 ? 10 : 8, ldc = i & 4 ? 9 : 8;
    fus += spmm::hybrid32_fusable(n, ldb, ldc, fake<const float>(8, i & 8 ? 8 : 0),
                                  fake<const float>(3, i & 16 ? 8 : 0),
                                  fake<const float>(4, i & 32 ? 4 : 0))
               ? '1'
               : '0';
  }
  spmm_trace::emit(fus);
  ++g_calls;
}

void grouped_grid() {
  section_begin();
  for (int W : {2, 4})
    for (int n : {0, 4, 128, 132, 260})
      for (int mb : {0, 1000})
        result(spmm::launch_bsrmm_grouped_f32(g_ctx, W, mb, n, (mb + W - 1) / W, kRowptr, kColind,
                                              kMasks, fake<const float>(2), fake<const float>(3),
                                              n, 1.f, 0.f, fake<float>(4), n));
  section_end("launch_bsrmm_grouped_f32");
  section_begin();
  for (int W : {2, 4, 8})
    for (int crow = 1; crow >= 0; --crow)
      for (int n : {0, 8, 256, 264})
        for (int ngroups : {0, 126})
          result(spmm::launch_bsrmm_grouped_f16(g_ctx, W, ngroups * W, n, ngroups, kRowptr,
                                                kColind, kMasks, fake<const unsigned>(2),
                                                fake<const uint16_t>(3), n, 1.f, 0.f,
                                                fake<float>(4), crow ? n : ngroups * W * 16,
                                                crow != 0));
  section_end("launch_bsrmm_grouped_f16");
}

void analysis_grid() {
  section_begin();
  for (int rowd = 1; rowd >= 0; --rowd)
    for (int nnzb : {0, 1, 4, 5, 100, 1 << 20})
      for (int col = 1; col >= 0; --col)
        result(spmm::launch_bsr32_analysis(g_ctx, rowd ? SPMM_DIRECTION_ROW : SPMM_DIRECTION_COLUMN,
                                           nnzb, fake<const float>(2), fake<unsigned>(5),
                                           col ? fake<float>(6) : nullptr));
  section_end("launch_bsr32_analysis");
  section_begin();
  for (int rowd = 1; rowd >= 0; --rowd)
    for (int nnzb : {0, 1, 100, 1 << 20})
      for (int col = 1; col >= 0; --col)
        result(spmm::launch_bsr16_analysis(g_ctx, rowd ? SPMM_DIRECTION_ROW : SPMM_DIRECTION_COLUMN,
                                           nnzb, fake<const uint16_t>(2), fake<unsigned>(5),
                                           col ? fake<uint16_t>(6) : nullptr));
  section_end("launch_bsr16_analysis");
}

constexpr int kCsrNs[] = {4, 8, 16, 32, 48, 64, 68, 128, 132, 256, 260};

// n x hot x both flags x (B, C aligned or off by 4 / 8 bytes) x leading dimensions
// (ldb = n, n + 1, n + 2 with ldc = n + 2; ldc = n otherwise) at one shape: alignment
// and leading dimensions crossed for the plain fp32 entry, one at a time for the hot and
// fp16 forms (the same pick_vec); then the grid sizing (rows, nnz hint, waves per CU) at three n
void csr_grid(bool f16) {
  void* ws = fake<void>(9);
  auto run = [&](int m, int n, int boff, int coff, int ldb, int ldc, int nnz, int hot) {
    if (f16)
      result(spmm::launch_csrmm_rowmajor_f16(g_ctx, m, n, kRowptr, kColind,
                                             fake<const uint16_t>(2), 0,
                                             fake<const uint16_t>(3, boff), ldb, 1.f, 0.f,
                                             fake<float>(4, coff), ldc, ws, nnz));
    else
      result(spmm::launch_csrmm_rowmajor(g_ctx, m, n, kRowptr, kColind, fake<const float>(2), 0,
                                         fake<const float>(3, boff), ldb, 1.f, 0.f,
                                         fake<float>(4, coff), ldc, ws, nnz, hot));
  };
  for (int n : kCsrNs)
    for (int hot = 0; hot < (f16 ? 1 : 3); ++hot)
      for (int flags : {0, (int)SPMM_CSR_NT_STREAMS, (int)SPMM_CSR_SEQUENTIAL_ROWS,
                        (int)(SPMM_CSR_NT_STREAMS | SPMM_CSR_SEQUENTIAL_ROWS)})
        for (int al = 0; al < 5; ++al)
          for (int ld = 0; ld < 3; ++ld) {
            if (al && ld && (f16 || hot)) continue;  // crossed for the plain fp32 entry only
            g_ctx->csr_flags = flags;
            const int boff = al == 1 ? 4 : (al == 2 ? 8 : 0), coff = al == 3 ? 4 : (al == 4 ? 8 : 0);
            run(4096, n, boff, coff, n + ld, n + (ld == 2 ? 2 : 0), 65536, hot);
          }
  g_ctx->csr_flags = SPMM_CSR_NT_STREAMS;
  for (int n : {64, 256})
    for (int hot = 0; hot < (f16 ? 1 : 2); ++hot)
      for (int wpc : {0, 8})
        for (int m : {100, 4096, 1 << 20})
          for (int nnz : {-1, 1 << 27}) {
            g_ctx->csr_waves_per_cu = wpc;
            run(m, n, 0, 0, n, n, nnz, hot);
          }
  run(0, 64, 0, 0, 64, 64, 0, 0);
  run(4096, 0, 0, 0, 0, 0, 0, 0);
  g_ctx->csr_waves_per_cu = 0;
}

void transpose_grid() {
  // tile rows on both sides of grid.y's 65535, and past 2^31 - 1 tiles in all
  const int rows[] = {0, 1, 64, 65, 65535 * 64, 65535 * 64 + 1, 0x7fffffff};
  section_begin();
  for (int r : rows)
    for (int c : {0, 64, 65, 4097})
      for (float beta : {0.f, 1.f})
        result(spmm::launch_transpose(g_ctx, r, c, fake<const float>(2), c, fake<float>(4), r,
                                      beta));
  section_end("launch_transpose");
  section_begin();
  for (int r : rows)
    for (int c : {0, 64, 65, 4097})
      result(spmm::launch_transpose16(g_ctx, r, c, fake<const uint16_t>(2), c, fake<uint16_t>(4),
                                      r));
  section_end("launch_transpose16");
}

// "cases" mode: one launcher call per input line, its launches' tags per output line
int run_cases() {
  g_cases = true;
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string kind;
    in >> kind;
    std::vector<long long> f;
    for (long long x; in >> x;) f.push_back(x);
    g_tags.clear();
    g_ctx->csr_flags = SPMM_CSR_NT_STREAMS;
    g_ctx->hybrid_flags = 0;
    if (kind == "bsr" && f.size() == 18) {
      BsrCase c;
      c.bs = f[1], c.n = f[2], c.rowd = f[3], c.brow = f[4], c.crow = f[5];
      c.voff = f[6], c.boff = f[7], c.coff = f[8];
      c.mb = f[11], c.kb = f[12], c.nnzb = f[13], c.masks = f[14], c.dense = f[15];
      c.bsr_flags = f[16], c.hybrid_flags = f[17];
      run_bsr(c, f[0] != 0, (int)f[9], (int)f[10]);
    } else if (kind == "csr" && f.size() == 10) {
      g_ctx->csr_flags = (int)f[9];
      void* ws = fake<void>(9);
      if (f[0])
        spmm::launch_csrmm_rowmajor_f16(g_ctx, f[1], f[2], kRowptr, kColind,
                                        fake<const uint16_t>(2), 0,
                                        fake<const uint16_t>(3, f[3]), f[5], 1.f, 0.f,
                                        fake<float>(4, f[4]), f[6], ws, f[7]);
      else
        spmm::launch_csrmm_rowmajor(g_ctx, f[1], f[2], kRowptr, kColind, fake<const float>(2), 0,
                                    fake<const float>(3, f[3]), f[5], 1.f, 0.f,
                                    fake<float>(4, f[4]), f[6], ws, f[7], (int)f[8]);
    } else if (kind == "hybrid" && f.size() == 5) {
      g_ctx->hybrid_flags = (int)f[4];
      spmm::launch_hybrid32_fused(g_ctx, f[0], f[1], 1.f, kRowptr, kColind, fake<const float>(2),
                                  fake<const int>(6), fake<const int>(7), fake<const float>(8),
                                  fake<const float>(3), f[2], 0.f, fake<float>(4), f[3]);
    } else {
      std::fprintf(stderr, "dispatch_trace cases: bad line: %s\n", line.c_str());
      return 2;
    }
    std::string out;
    for (const std::string& t : g_tags) out += (out.empty() ? "" : " ") + t;
    std::printf("%s\n", out.c_str());
  }
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  spmm_context ctx;
  ctx.num_cus = 256;
  g_ctx = &ctx;
  if (argc > 1 && !std::strcmp(argv[1], "cases")) {
    const int rc = run_cases();
    std::free(ctx.scratch);
    std::free(ctx.order);
    std::free(ctx.tickets);
    return rc;
  }

  section_begin();
  bsr_grid(false);
  section_end("launch_bsrmm_f32");
  section_begin();
  bsr_grid(true);
  section_end("launch_bsrmm_f16");
  section_begin();
  hybrid_grid();
  section_end("launch_hybrid32_fused");
  grouped_grid();
  analysis_grid();

  section_begin();
  csr_grid(false);
  section_end("launch_csrmm_rowmajor");
  section_begin();
  csr_grid(true);
  section_end("launch_csrmm_rowmajor_f16");
  section_begin();
  for (int k : {1, 1000, 1 << 22})
    for (long long nnz : {0ll, 100ll, 1ll << 33})
      result(spmm::launch_csr_hot_analysis(g_ctx, k, nnz, kColind, 0, 300, fake<int>(6)));
  section_end("launch_csr_hot_analysis");
  transpose_grid();

  std::free(ctx.scratch);
  std::free(ctx.order);
  std::free(ctx.tickets);
  return 0;
}
