// host_sanitize.cpp — the host forms, converters, reorderers, generators and loaders of
// prep.cpp, host_data.cpp, host_io.cpp and reorder.cpp under AddressSanitizer +
// UndefinedBehaviorSanitizer (bin/host_asan) and ThreadSanitizer (bin/host_tsan).
//
//   host_sanitize <group> <tmpdir>     prints "ok <case>" per case, exit status 0
//
// What this sees that the Python host tests cannot: every operand is its own
// malloc of exactly the bytes the contract lets the entry touch, so the allocator's redzones
// sit on both ends; the padding columns of a padded operand and the positions outside a
// view are poisoned; the refusals run on fully poisoned outputs. A stray read or write is a
// report, not the same bits. The threaded legs run every entry that has workers at the
// smallest size with two of them, once with OMP_NUM_THREADS=1 and once with 7, and the two
// results must be memcmp-equal. Numerics stay in the Python host tests: this driver asserts
// statuses, thread-count equality and exact round trips only.
//
// A new case: add it to its group's function and its name to tests/test_host_sanitize.py.
#include <sanitizer/asan_interface.h>
#include <sys/stat.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <set>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "spmm_hip.h"
#include "spmm_host.h"
#include "spmm_reorder.h"

namespace {

std::string g_case;

[[noreturn]] void fail(int line, const char* what) {
  std::fprintf(stderr, "FAIL %s: %s (host_sanitize.cpp:%d)\n", g_case.c_str(), what, line);
  std::exit(1);
}
#define REQUIRE(c)                      \
  do {                                  \
    if (!(c)) fail(__LINE__, #c);       \
  } while (0)
#define SUCCEEDS(e) REQUIRE((e) == SPMM_STATUS_SUCCESS)
#define REFUSES(e) REQUIRE((e) == SPMM_STATUS_INVALID_VALUE)

void ok(const std::string& name) {
  std::printf("ok %s\n", name.c_str());
  std::fflush(stdout);
}

#if defined(__SANITIZE_ADDRESS__)
bool is_poisoned(const void* p) { return __asan_address_is_poisoned(p) != 0; }
constexpr bool kAsan = true;
#else
bool is_poisoned(const void*) { return true; }  // nothing is poisoned under TSan
constexpr bool kAsan = false;
#endif

// ------------------------------------------------------------------ operands
// n elements in a malloc of exactly n * sizeof(T) bytes (n = 0: one byte, poisoned).
template <typename T>
class Block {
 public:
  explicit Block(size_t n) : n_(n), p_(static_cast<T*>(std::malloc(bytes()))) {
    REQUIRE(p_ != nullptr);
    if (n_ == 0) ASAN_POISON_MEMORY_REGION(p_, 1);
  }
  Block(Block&& o) noexcept : n_(o.n_), p_(o.p_) { o.p_ = nullptr; }
  Block(const Block&) = delete;
  Block& operator=(const Block&) = delete;
  ~Block() {
    if (!p_) return;
    ASAN_UNPOISON_MEMORY_REGION(p_, bytes());
    std::free(p_);
  }
  T* get() const { return p_; }
  size_t size() const { return n_; }
  T& operator[](size_t i) const { return p_[i]; }
  // Poisons the elements [lo, hi). ASan poisons whole 8-byte granules, or a granule's tail
  // when what follows is poisoned too, so a short run may keep an accessible word.
  void poison(size_t lo, size_t hi) const {
    if (hi > lo) ASAN_POISON_MEMORY_REGION(p_ + lo, (hi - lo) * sizeof(T));
  }
  void poison_all() const { poison(0, n_); }

 private:
  size_t bytes() const { return n_ ? n_ * sizeof(T) : 1; }
  size_t n_;
  T* p_;
};

using Bytes = std::vector<unsigned char>;
template <typename T>
void put(Bytes& o, const T* p, size_t n) {
  const unsigned char* b = reinterpret_cast<const unsigned char*>(p);
  o.insert(o.end(), b, b + n * sizeof(T));
}

inline uint32_t hash32(uint64_t i) {
  uint64_t x = (i + 1) * 0x9E3779B97F4A7C15ull;
  x ^= x >> 29;
  x *= 0xBF58476D1CE4E5B9ull;
  return (uint32_t)(x >> 32);
}
float gen_f32(uint64_t i) { return (float)(hash32(i) >> 8) * (1.f / 8388608.f) - 1.f; }      // [-1, 1)
float gen_pos(uint64_t i) { return 1.f + (float)(hash32(i) >> 9) * (1.f / 8388608.f); }      // [1, 2)
uint16_t gen_f16(uint64_t i) {  // finite binary16, exponents around 1
  const uint32_t h = hash32(i);
  return (uint16_t)((h & 0x83ffu) | (((h >> 10) % 9 + 10) << 10));
}
uint16_t gen_bf16(uint64_t i) {  // finite bfloat16, exponents around 1
  const uint32_t h = hash32(i);
  return (uint16_t)((h & 0x807fu) | (((h >> 7) % 10 + 120) << 7));
}

// rows x n at leading dimension ld in exactly (rows - 1) * ld + n elements, the padding
// columns between the rows poisoned.
template <typename T>
struct Dense {
  int64_t rows, n, ld;
  Block<T> b;
  template <typename G>
  Dense(int64_t rows_, int64_t n_, int64_t ld_, G gen)
      : rows(rows_), n(n_), ld(ld_), b(rows_ > 0 && n_ > 0 ? (size_t)((rows_ - 1) * ld_ + n_) : 0) {
    for (size_t i = 0; i < b.size(); ++i) b[i] = gen(i);
    for (int64_t r = 0; r + 1 < rows && n > 0; ++r) b.poison((size_t)(r * ld + n), (size_t)((r + 1) * ld));
  }
  T* get() const { return b.get(); }
  void snap(Bytes& o) const {
    for (int64_t r = 0; r < rows && n > 0; ++r) put(o, b.get() + r * ld, (size_t)n);
  }
};

struct Pattern {
  std::vector<int> len;  // row lengths
  int k;                 // columns
};

struct Lay {
  const char* name;
  int pad, base;
  bool view;
};
const Lay kLays[] = {{"tight/base0", 0, 0, false}, {"padded/base0", 3, 0, false},
                     {"tight/base1", 0, 1, false}, {"padded/base1", 3, 1, false},
                     {"tight/base0/view", 0, 0, true}, {"padded/base1/view", 3, 1, true}};

// A CSR pattern in exact-size arrays: unsorted columns with duplicates (sorted on request).
// A view has `front` foreign positions before the matrix's and `back` after them; they are
// poisoned in the column indices and in every per-edge array.
struct Csr {
  int m, k, nnz, front, back, base;
  Block<int> rp, ci;
  int nnz_arg() const { return front + nnz + back; }
  spmm_index_base_t ib() const { return base ? SPMM_INDEX_BASE_ONE : SPMM_INDEX_BASE_ZERO; }
};

Csr make_csr(const Pattern& p, int base, bool view, bool sorted = false) {
  const int m = (int)p.len.size();
  int nnz = 0;
  for (int l : p.len) nnz += l;
  const int front = view ? 3 : 0, back = view ? 2 : 0;
  Csr a{m, p.k, nnz, front, back, base, Block<int>((size_t)m + 1),
        Block<int>((size_t)(front + nnz + back))};
  int pos = front;
  a.rp[0] = pos + base;
  for (int r = 0; r < m; ++r) {
    for (int j = 0; j < p.len[r]; ++j)
      a.ci[(size_t)(pos + j)] = (int)(((int64_t)r * 31 + (j / 2) * 17 + (j % 3) * 5) % p.k) + base;
    if (sorted) std::sort(a.ci.get() + pos, a.ci.get() + pos + p.len[r]);
    pos += p.len[r];
    a.rp[(size_t)r + 1] = pos + base;
  }
  a.ci.poison(0, (size_t)front);
  a.ci.poison((size_t)(front + nnz), a.ci.size());
  return a;
}

// A per-edge array of `per` elements per position over the pattern's positions.
template <typename T>
struct Edge {
  size_t lo, hi;
  Block<T> b;
  template <typename G>
  Edge(const Csr& a, int per, G gen)
      : lo((size_t)a.front * per), hi((size_t)(a.front + a.nnz) * per), b((size_t)a.nnz_arg() * per) {
    for (size_t i = lo; i < hi; ++i) b[i] = gen(i);
    b.poison(0, lo);
    b.poison(hi, b.size());
  }
  T* get() const { return b.get(); }
  void snap(Bytes& o) const { put(o, b.get() + lo, hi - lo); }
};

void check_setup() {
  if (!kAsan) return;
  const Dense<float> d(3, 5, 8, gen_f32);  // rows of 5 floats, 3 padding words
  bool any = false;
  for (int c = 5; c < 8; ++c) any = any || is_poisoned(d.get() + c);
  REQUIRE(any);
  REQUIRE(!is_poisoned(d.get() + 4) && !is_poisoned(d.get() + 8));
  REQUIRE(is_poisoned(reinterpret_cast<const char*>(d.get() + d.b.size())));  // behind the block
  REQUIRE(is_poisoned(reinterpret_cast<const char*>(d.get()) - 1));           // before it
  const Csr a = make_csr({{2, 0, 3}, 4}, 1, true);
  const Edge<float> e(a, 1, gen_f32);
  REQUIRE(is_poisoned(e.get()) && is_poisoned(e.get() + e.b.size() - 1));
  REQUIRE(!is_poisoned(e.get() + e.lo) && !is_poisoned(e.get() + e.hi - 1));
  REQUIRE(is_poisoned(a.ci.get()) && !is_poisoned(a.ci.get() + a.front));
  const Block<int> z(0);
  REQUIRE(is_poisoned(z.get()));
}

// ------------------------------------------------------------------ the host forms
// Every op builds its operands for (pattern, width, layout, heads), calls the entry and
// returns the bytes of its outputs' valid parts.
using Op = Bytes (*)(const Pattern&, int, const Lay&, int);

Bytes op_sddmm(const Pattern& p, int w, const Lay& l, int) {
  const Csr a = make_csr(p, l.base, l.view);
  const Dense<float> X(a.m, w, w + l.pad, gen_f32), Y(a.k, w, w + l.pad, gen_pos);
  const Edge<float> out(a, 1, gen_f32);
  const float* x = w ? X.get() : nullptr;  // X and Y may be NULL when n == 0
  const float* y = w ? Y.get() : nullptr;
  for (float beta : {0.f, 0.5f})
    SUCCEEDS(spmm_sddmm_csr_host_f32(a.m, w, a.k, a.nnz_arg(), 1.5f, a.rp.get(), a.ci.get(), a.ib(), x,
                                     w + l.pad, y, w + l.pad, beta, out.get()));
  Bytes o;
  out.snap(o);
  return o;
}

Bytes op_softmax(const Pattern& p, int, const Lay& l, int heads, bool multi) {
  const Csr a = make_csr(p, l.base, l.view);
  const Edge<float> x(a, heads, gen_f32), y(a, heads, gen_f32);
  if (multi) {
    SUCCEEDS(spmm_edge_softmax_csr_heads_host_f32(a.m, a.nnz_arg(), heads, a.rp.get(), a.ib(), x.get(), y.get()));
    SUCCEEDS(spmm_edge_softmax_csr_heads_host_f32(a.m, a.nnz_arg(), heads, a.rp.get(), a.ib(), x.get(), x.get()));
  } else {
    SUCCEEDS(spmm_edge_softmax_csr_host_f32(a.m, a.nnz_arg(), a.rp.get(), a.ib(), x.get(), y.get()));
    SUCCEEDS(spmm_edge_softmax_csr_host_f32(a.m, a.nnz_arg(), a.rp.get(), a.ib(), x.get(), x.get()));
  }
  Bytes o;
  y.snap(o);
  x.snap(o);
  return o;
}
Bytes op_softmax_fwd(const Pattern& p, int w, const Lay& l, int) { return op_softmax(p, w, l, 1, false); }
Bytes op_softmax_heads_fwd(const Pattern& p, int w, const Lay& l, int h) { return op_softmax(p, w, l, h, true); }

Bytes op_softmax_b(const Pattern& p, int, const Lay& l, int heads, bool multi) {
  const Csr a = make_csr(p, l.base, l.view);
  const Edge<float> y(a, heads, gen_pos), g(a, heads, gen_f32), gx(a, heads, gen_f32);
  if (multi) {
    SUCCEEDS(spmm_edge_softmax_bwd_csr_heads_host_f32(a.m, a.nnz_arg(), heads, a.rp.get(), a.ib(), y.get(), g.get(), gx.get()));
    SUCCEEDS(spmm_edge_softmax_bwd_csr_heads_host_f32(a.m, a.nnz_arg(), heads, a.rp.get(), a.ib(), y.get(), g.get(), g.get()));
  } else {
    SUCCEEDS(spmm_edge_softmax_bwd_csr_host_f32(a.m, a.nnz_arg(), a.rp.get(), a.ib(), y.get(), g.get(), gx.get()));
    SUCCEEDS(spmm_edge_softmax_bwd_csr_host_f32(a.m, a.nnz_arg(), a.rp.get(), a.ib(), y.get(), g.get(), g.get()));
  }
  Bytes o;
  gx.snap(o);
  g.snap(o);
  return o;
}
Bytes op_softmax_bwd(const Pattern& p, int w, const Lay& l, int) { return op_softmax_b(p, w, l, 1, false); }
Bytes op_softmax_heads_bwd(const Pattern& p, int w, const Lay& l, int h) { return op_softmax_b(p, w, l, h, true); }

Bytes op_sddmm_heads(const Pattern& p, int d, const Lay& l, int heads) {
  const Csr a = make_csr(p, l.base, l.view);
  const int ld = heads * d + l.pad;
  const Dense<float> X(a.m, heads * d, ld, gen_f32), Y(a.k, heads * d, ld, gen_pos);
  const Edge<float> out(a, heads, gen_f32);
  for (float beta : {0.f, 0.5f})
    SUCCEEDS(spmm_sddmm_csr_heads_host_f32(a.m, d, a.k, a.nnz_arg(), heads, 1.5f, a.rp.get(), a.ci.get(), a.ib(),
                                           d ? X.get() : nullptr, ld, d ? Y.get() : nullptr, ld, beta, out.get()));
  Bytes o;
  out.snap(o);
  return o;
}

template <bool BF16>
Bytes op_sddmm_heads_half(const Pattern& p, int d, const Lay& l, int heads) {
  const Csr a = make_csr(p, l.base, l.view);
  const int ld = heads * d + l.pad;
  const auto gen = BF16 ? gen_bf16 : gen_f16;
  const Dense<uint16_t> X(a.m, heads * d, ld, gen), Y(a.k, heads * d, ld, gen);
  const Edge<float> out(a, heads, gen_f32);
  for (float beta : {0.f, 0.5f})
    SUCCEEDS((BF16 ? spmm_sddmm_csr_heads_host_bf16 : spmm_sddmm_csr_heads_host_f16)(
        a.m, d, a.k, a.nnz_arg(), heads, 1.5f, a.rp.get(), a.ci.get(), a.ib(), d ? X.get() : nullptr, ld,
        d ? Y.get() : nullptr, ld, beta, out.get()));
  Bytes o;
  out.snap(o);
  return o;
}

Bytes op_csrmm_heads(const Pattern& p, int d, const Lay& l, int heads) {
  const Csr a = make_csr(p, l.base, l.view);
  const int ld = heads * d + l.pad;
  const Dense<float> B(a.k, heads * d, ld, gen_f32), C(a.m, heads * d, ld, gen_f32);
  const Edge<float> val(a, heads, gen_pos);
  for (float beta : {0.f, 0.5f})
    SUCCEEDS(spmm_csrmm_heads_host_f32(a.m, d, a.k, a.nnz_arg(), heads, 1.5f, a.rp.get(), a.ci.get(), val.get(),
                                       a.ib(), B.get(), ld, beta, C.get(), ld));
  Bytes o;
  C.snap(o);
  return o;
}

template <bool BF16>
Bytes op_csrmm_heads_half(const Pattern& p, int d, const Lay& l, int heads) {
  const Csr a = make_csr(p, l.base, l.view);
  const int ld = heads * d + l.pad;
  const Dense<uint16_t> B(a.k, heads * d, ld, BF16 ? gen_bf16 : gen_f16);
  const Dense<float> C(a.m, heads * d, ld, gen_f32);
  const Edge<float> val(a, heads, gen_pos);
  for (float beta : {0.f, 0.5f})
    SUCCEEDS((BF16 ? spmm_csrmm_heads_host_bf16 : spmm_csrmm_heads_host_f16)(
        a.m, d, a.k, a.nnz_arg(), heads, 1.5f, a.rp.get(), a.ci.get(), val.get(), a.ib(), B.get(), ld, beta,
        C.get(), ld));
  Bytes o;
  C.snap(o);
  return o;
}

// Forward with values and the winners, and the unweighted forward without them.
Bytes op_reduce_fwd(const Pattern& p, int n, const Lay& l, int) {
  const Csr a = make_csr(p, l.base, l.view);
  const int ld = n + l.pad;
  const Dense<float> B(a.k, n, ld, gen_f32), C(a.m, n, ld, gen_f32), C2(a.m, n, ld, gen_f32);
  const Dense<int> arg(a.m, n, ld, hash32);
  const Edge<float> val(a, 1, gen_f32);
  SUCCEEDS(spmm_csrmm_reduce_host_f32(SPMM_REDUCE_MAX, a.m, n, a.k, a.nnz_arg(), a.rp.get(), a.ci.get(), val.get(),
                                      a.ib(), B.get(), ld, C.get(), ld, arg.get(), ld));
  SUCCEEDS(spmm_csrmm_reduce_host_f32(SPMM_REDUCE_MIN, a.m, n, a.k, a.nnz_arg(), a.rp.get(), a.ci.get(), nullptr,
                                      a.ib(), B.get(), ld, C2.get(), ld, nullptr, 0));
  Bytes o;
  C.snap(o);
  arg.snap(o);
  C2.snap(o);
  return o;
}

// The transpose's arrays from spmm_csr2csc, the winners from the forward, then the backward
// with and without values.
Bytes op_reduce_bwd(const Pattern& p, int n, const Lay& l, int) {
  const Csr a = make_csr(p, l.base, l.view);
  const int ld = n + l.pad;
  const Block<int> trp((size_t)a.k + 1), tci((size_t)a.nnz), perm((size_t)a.nnz);
  SUCCEEDS(spmm_csr2csc(a.m, a.k, a.nnz, nullptr, a.rp.get(), a.ci.get(), 0, a.ib(), a.ib(), nullptr, trp.get(),
                        tci.get(), perm.get()));
  const Dense<float> B(a.k, n, ld, gen_f32), C(a.m, n, ld, gen_f32), dC(a.m, n, ld, gen_f32);
  const Dense<float> dB(a.k, n, ld, gen_f32), dB2(a.k, n, ld, gen_f32);
  const Dense<int> arg(a.m, n, ld, hash32);
  const Edge<float> val(a, 1, gen_f32);
  SUCCEEDS(spmm_csrmm_reduce_host_f32(SPMM_REDUCE_MAX, a.m, n, a.k, a.nnz_arg(), a.rp.get(), a.ci.get(), val.get(),
                                      a.ib(), B.get(), ld, C.get(), ld, arg.get(), ld));
  SUCCEEDS(spmm_csrmm_reduce_bwd_host_f32(a.k, n, a.m, a.nnz_arg(), trp.get(), tci.get(), perm.get(), val.get(),
                                          a.ib(), dC.get(), ld, arg.get(), ld, dB.get(), ld));
  SUCCEEDS(spmm_csrmm_reduce_bwd_host_f32(a.k, n, a.m, a.nnz_arg(), trp.get(), tci.get(), perm.get(), nullptr,
                                          a.ib(), dC.get(), ld, arg.get(), ld, dB2.get(), ld));
  Bytes o;
  dB.snap(o);
  dB2.snap(o);
  return o;
}

// Every value width with and without perm, both output bases; then csr2csc applied twice
// gives the matrix back with every row stably sorted by column.
Bytes op_csr2csc(const Pattern& p, int, const Lay& l, int) {
  const Csr a = make_csr(p, l.base, l.view);
  Bytes o;
  for (int vb : {0, 2, 4, 8})
    for (int bc : {0, 1}) {
      const bool with_perm = (vb / 2 + bc) % 2 == 0;
      const Edge<unsigned char> val(a, std::max(vb, 1), [](uint64_t i) { return (unsigned char)hash32(i); });
      const Block<unsigned char> tval((size_t)a.nnz * vb);
      const Block<int> tcp((size_t)a.k + 1), tri((size_t)a.nnz), perm(with_perm ? (size_t)a.nnz : 0);
      SUCCEEDS(spmm_csr2csc(a.m, a.k, a.nnz, vb ? val.get() : nullptr, a.rp.get(), a.ci.get(), vb, a.ib(),
                            bc ? SPMM_INDEX_BASE_ONE : SPMM_INDEX_BASE_ZERO, vb ? tval.get() : nullptr,
                            tcp.get(), tri.get(), with_perm ? perm.get() : nullptr));
      put(o, tcp.get(), tcp.size());
      put(o, tri.get(), tri.size());
      put(o, tval.get(), tval.size());
      put(o, perm.get(), perm.size());
    }
  // twice: the values are the positions, so the stable order is visible
  const Edge<int> pos(a, 1, [](uint64_t i) { return (int)i; });
  const Block<int> tcp((size_t)a.k + 1), tri((size_t)a.nnz), tpos((size_t)a.nnz);
  const Block<int> rp2((size_t)a.m + 1), ci2((size_t)a.nnz), pos2((size_t)a.nnz);
  SUCCEEDS(spmm_csr2csc(a.m, a.k, a.nnz, pos.get(), a.rp.get(), a.ci.get(), 4, a.ib(), SPMM_INDEX_BASE_ONE,
                        tpos.get(), tcp.get(), tri.get(), nullptr));
  SUCCEEDS(spmm_csr2csc(a.k, a.m, a.nnz, tpos.get(), tcp.get(), tri.get(), 4, SPMM_INDEX_BASE_ONE, a.ib(),
                        pos2.get(), rp2.get(), ci2.get(), nullptr));
  std::vector<int> order;
  for (int r = 0; r < a.m; ++r) {
    const int b = a.rp[(size_t)r] - a.base, e = a.rp[(size_t)r + 1] - a.base;
    REQUIRE(rp2[(size_t)r] == b - a.front + a.base && rp2[(size_t)r + 1] == e - a.front + a.base);
    order.resize((size_t)(e - b));
    for (int j = b; j < e; ++j) order[(size_t)(j - b)] = j;
    std::stable_sort(order.begin(), order.end(),
                     [&](int x, int y) { return a.ci[(size_t)x] < a.ci[(size_t)y]; });
    for (int j = b; j < e; ++j) {
      REQUIRE(ci2[(size_t)(j - a.front)] == a.ci[(size_t)order[(size_t)(j - b)]]);
      REQUIRE(pos2[(size_t)(j - a.front)] == order[(size_t)(j - b)]);
    }
  }
  return o;
}

struct OpEntry {
  const char* name;
  Op op;
  bool widths, heads;
};
const OpEntry kOps[] = {
    {"sddmm", op_sddmm, true, false},
    {"softmax_fwd", op_softmax_fwd, false, false},
    {"softmax_bwd", op_softmax_bwd, false, false},
    {"sddmm_heads_f32", op_sddmm_heads, true, true},
    {"softmax_heads_fwd", op_softmax_heads_fwd, false, true},
    {"softmax_heads_bwd", op_softmax_heads_bwd, false, true},
    {"csrmm_heads_f32", op_csrmm_heads, true, true},
    {"sddmm_heads_f16", op_sddmm_heads_half<false>, true, true},
    {"sddmm_heads_bf16", op_sddmm_heads_half<true>, true, true},
    {"csrmm_heads_f16", op_csrmm_heads_half<false>, true, true},
    {"csrmm_heads_bf16", op_csrmm_heads_half<true>, true, true},
    {"reduce_fwd", op_reduce_fwd, true, false},
    {"reduce_bwd", op_reduce_bwd, true, false},
    {"csr2csc", op_csr2csc, false, false},
};

struct NamedPattern {
  const char* name;
  Pattern p;
  std::vector<int> widths;  // n, or d per head; 0 is the empty width
};
// Row lengths on each rule's boundaries: the softmax's 64 chains and pieces of 1024, the
// product's and the reducers' pieces of 128. The long rows run the widths that take another
// path in the dot (G = 1, 2 and 64 chains), the short ones every width.
const NamedPattern kPatterns[] = {
    {"empty_rows", {{0, 0, 3, 1, 0, 0, 0, 7, 2, 0}, 6}, {0, 1, 4, 5, 37, 260}},
    {"m0", {{}, 4}, {0, 5}},
    {"nnz0", {{0, 0, 0, 0, 0}, 4}, {0, 5}},
    {"softmax_lengths", {{63, 0, 64, 65, 1023, 0, 0, 1024, 1025, 2049}, 11}, {1, 5, 260}},
    {"reduce_lengths", {{127, 128, 0, 129, 1}, 9}, {1, 4, 5, 37, 260}},
};

void group_forms() {
  for (const OpEntry& op : kOps)
    for (const NamedPattern& np : kPatterns) {
      const std::string name = std::string(op.name) + "." + np.name;
      for (const Lay& l : kLays)
        for (int w : op.widths ? np.widths : std::vector<int>{1})
          for (int heads : op.heads ? std::vector<int>{1, 3} : std::vector<int>{1}) {
            g_case = name + " " + l.name + " width " + std::to_string(w) + " heads " + std::to_string(heads);
            op.op(np.p, w, l, heads);
          }
      ok(name);
    }
}

// ------------------------------------------------------------------ threaded legs
// The smallest sizes with two workers, from csrc/host_util.hpp and csrc/host_io.cpp:
//   parallel_for(n)          min(threads, max(1, n / 4096)) workers: n = 8192 rows, block rows,
//                            positions or nodes;
//   spmm_csr2csc's fill      nnz / 65536 workers: nnz = 131072;
//   parse_ints               (bytes >> 20) + 1 workers: a text just over 1 MiB;
//   spmm_hybrid_plan         num_threads() workers at every size.
// 8192 rows of 16 positions serve the ops (131072 positions); 32 positions a row make the
// text of the column indices 1.2 MiB and serve the rest. write_ints and the checksum give parallel_for their count of
// 1 MiB chunks, so two workers would take 2^33 values: their legs run with one worker. So
// does spmm_block_heatmap's: 8192 block rows are an output of 8192^2 ints (256 MiB).
Pattern big_pattern(int n, int per) { return {std::vector<int>((size_t)n, per), n}; }
constexpr int kBigN = 8192, kBigPer = 32;

void both_thread_counts(const std::string& name, const std::function<Bytes()>& run) {
  g_case = name;
  setenv("OMP_NUM_THREADS", "1", 1);
  const Bytes one = run();
  setenv("OMP_NUM_THREADS", "7", 1);
  const Bytes seven = run();
  REQUIRE(one.size() == seven.size());
  REQUIRE(one.empty() || std::memcmp(one.data(), seven.data(), one.size()) == 0);
  ok(name);
}

std::string slurp(const std::string& path) {
  std::string s;
  FILE* f = std::fopen(path.c_str(), "rb");
  REQUIRE(f != nullptr);
  char buf[1 << 16];
  size_t got;
  while ((got = std::fread(buf, 1, sizeof buf, f)) > 0) s.append(buf, got);
  std::fclose(f);
  return s;
}

void spit(const std::string& path, const std::string& text) {
  FILE* f = std::fopen(path.c_str(), "wb");
  REQUIRE(f != nullptr);
  REQUIRE(std::fwrite(text.data(), 1, text.size(), f) == text.size());
  REQUIRE(std::fclose(f) == 0);
}

Bytes conv_csr2bsr(const Csr& a, int m, int n, int bs, spmm_direction_t dir, bool back);
Bytes conv_divide(const Csr& a, int bs, float density);
Bytes conv_reorder(const Csr& a, int which);

void group_threads(const std::string& tmp) {
  const Pattern big = big_pattern(kBigN, kBigPer / 2);
  const Lay tight = kLays[0];
  for (const OpEntry& op : kOps)
    both_thread_counts(std::string("threads.") + op.name, [&] { return op.op(big, 4, tight, 2); });
  const Csr a = make_csr(big_pattern(kBigN, kBigPer), 0, false, true);
  both_thread_counts("threads.csr2bsr", [&] { return conv_csr2bsr(a, kBigN, kBigN, 1, SPMM_DIRECTION_ROW, false); });
  {
    const Csr wide = make_csr(big_pattern(2 * kBigN, 8), 0, false, true);
    both_thread_counts("threads.divide", [&] { return conv_divide(wide, 2, 0.5f); });
    both_thread_counts("threads.hybrid_plan", [&] {
      float density = 0;
      int64_t nnzb = 0, rest = 0;
      double est = 0;
      SUCCEEDS(spmm_hybrid_plan(wide.m, wide.rp.get(), wide.ci.get(), 2, 64, 4, 0, 0, &density, &nnzb, &rest, &est));
      Bytes o;
      put(o, &density, 1);
      put(o, &nnzb, 1);
      put(o, &rest, 1);
      put(o, &est, 1);
      return o;
    });
  }
  for (int which = 0; which < 5; ++which) {
    static const char* names[] = {"reorder_degree", "reorder_bfs", "reorder_rcm", "permute_csr", "block_metrics"};
    both_thread_counts(std::string("threads.") + names[which], [&] { return conv_reorder(a, which); });
  }
  both_thread_counts("threads.text_csr", [&] {
    const std::string prefix = tmp + "/big";
    REQUIRE(spmm_host_dump_csr(prefix.c_str(), a.m, a.nnz, a.rp.get(), a.ci.get()) == 0);
    const std::string text = slurp(prefix + "_indices.txt");
    REQUIRE(text.size() > (1u << 20) + 16);  // two parse workers
    int *rp = nullptr, *ci = nullptr, n = 0;
    int64_t nnz = 0;
    REQUIRE(spmm_host_load_csr(prefix.c_str(), &rp, &ci, &n, &nnz) == 0);
    REQUIRE(n == a.m && nnz == a.nnz);
    REQUIRE(std::memcmp(rp, a.rp.get(), sizeof(int) * ((size_t)n + 1)) == 0);
    REQUIRE(std::memcmp(ci, a.ci.get(), sizeof(int) * (size_t)nnz) == 0);
    Bytes o;
    put(o, text.data(), text.size());
    put(o, rp, (size_t)n + 1);
    put(o, ci, (size_t)nnz);
    spmm_host_free(rp);
    spmm_host_free(ci);
    return o;
  });
  both_thread_counts("threads.edge_list", [&] {
    std::string text = std::to_string(a.m) + " " + std::to_string(a.nnz) + "\n";
    for (int r = a.m - 1; r >= 0; --r)  // sources descending, destinations as stored
      for (int j = a.rp[(size_t)r]; j < a.rp[(size_t)r + 1]; ++j)
        text += std::to_string(r) + "\t" + std::to_string(a.ci[(size_t)(a.rp[(size_t)r] + a.rp[(size_t)r + 1] - 1 - j)]) + "\n";
    REQUIRE(text.size() > (1u << 20) + 32);
    spit(tmp + "/big_edges.txt", text);
    int *rp = nullptr, *ci = nullptr, n = 0;
    int64_t nnz = 0;
    REQUIRE(spmm_host_load_graph((tmp + "/big_edges.txt").c_str(), &rp, &ci, &n, &nnz) == 0);
    REQUIRE(n == a.m && nnz == a.nnz);
    REQUIRE(std::memcmp(rp, a.rp.get(), sizeof(int) * ((size_t)n + 1)) == 0);
    REQUIRE(std::memcmp(ci, a.ci.get(), sizeof(int) * (size_t)nnz) == 0);  // sorted again
    Bytes o;
    put(o, rp, (size_t)n + 1);
    put(o, ci, (size_t)nnz);
    spmm_host_free(rp);
    spmm_host_free(ci);
    return o;
  });
  both_thread_counts("threads.binary_csr", [&] {
    const std::string path = tmp + "/big.csrbin";
    REQUIRE(spmm_host_save_csr_bin(path.c_str(), a.m, a.nnz, a.rp.get(), a.ci.get(), nullptr) == 0);
    int *rp = nullptr, *ci = nullptr, n = 0;
    int64_t nnz = 0;
    REQUIRE(spmm_host_load_csr_bin(path.c_str(), &rp, &ci, nullptr, &n, &nnz) == 0);
    const std::string file = slurp(path);
    Bytes o;
    put(o, file.data(), file.size());
    put(o, rp, (size_t)n + 1);
    put(o, ci, (size_t)nnz);
    spmm_host_free(rp);
    spmm_host_free(ci);
    return o;
  });
  both_thread_counts("threads.gen_powerlaw", [&] {
    int *rp = nullptr, *ci = nullptr;
    REQUIRE(spmm_host_gen_powerlaw_csr(kBigN, 40000, 300, 2.3, 11, &rp, &ci) == 0);
    REQUIRE(rp[kBigN] == 40000);
    Bytes o;
    put(o, rp, (size_t)kBigN + 1);
    put(o, ci, 40000);
    spmm_host_free(rp);
    spmm_host_free(ci);
    return o;
  });
  both_thread_counts("threads.gen_community", [&] {
    int *rp = nullptr, *ci = nullptr;
    int64_t nnz = 0;
    REQUIRE(spmm_host_gen_community_csr(kBigN, 6.0, 16, 64, 0.8, 5, &rp, &ci, &nnz) == 0);
    REQUIRE(rp[kBigN] == nnz);
    Bytes o;
    put(o, rp, (size_t)kBigN + 1);
    put(o, ci, (size_t)nnz);
    spmm_host_free(rp);
    spmm_host_free(ci);
    return o;
  });
  // The shared generator behind its mutex, drawn from two threads at once.
  g_case = "threads.shared_generator";
  {
    spmm_host_rng_seed(1234);
    const Block<float> x(4096), y(4096);
    std::thread t1([&] { spmm_host_random_array(4096, -1.f, 1.f, x.get()); });
    std::thread t2([&] { spmm_host_random_array(4096, -1.f, 1.f, y.get()); });
    t1.join();
    t2.join();
  }
  ok("threads.shared_generator");
}

// ------------------------------------------------------------------ converters and planners
// csr2bsr (sizes, then fill) on exact-size outputs; with `back`, bsr2csr of the result and
// the nonzero pattern compared with the input's.
Bytes conv_csr2bsr(const Csr& a, int m, int n, int bs, spmm_direction_t dir, bool back) {
  const int mb = (m + bs - 1) / bs, nb = (n + bs - 1) / bs;
  const Edge<float> val(a, 1, gen_pos);
  const Block<int> brp((size_t)mb + 1);
  int nnzb = -1;
  SUCCEEDS(spmm_xcsr2bsr_nnz(dir, m, n, a.rp.get(), a.ci.get(), bs, brp.get(), &nnzb));
  REQUIRE(nnzb >= 0 && brp[(size_t)mb] == nnzb);
  const Block<int> bci((size_t)nnzb);
  const Block<float> bval((size_t)nnzb * bs * bs);
  SUCCEEDS(spmm_scsr2bsr(dir, m, n, val.get(), a.rp.get(), a.ci.get(), bs, brp.get(), bval.get(), bci.get()));
  Bytes o;
  put(o, brp.get(), brp.size());
  put(o, bci.get(), bci.size());
  put(o, bval.get(), bval.size());
  if (!back) return o;
  const Block<int> crp((size_t)mb * bs + 1), cci((size_t)nnzb * bs * bs);
  const Block<float> cval((size_t)nnzb * bs * bs);
  SUCCEEDS(spmm_sbsr2csr(dir, mb, nb, bval.get(), brp.get(), bci.get(), bs, cval.get(), crp.get(), cci.get()));
  REQUIRE(crp[(size_t)mb * bs] == nnzb * bs * bs);
  std::set<std::pair<int, int>> want, got;
  for (int r = 0; r < m; ++r)
    for (int j = a.rp[(size_t)r] - a.base; j < a.rp[(size_t)r + 1] - a.base; ++j)
      want.insert({r, a.ci[(size_t)j] - a.base});
  for (int r = 0; r < mb * bs; ++r)
    for (int j = crp[(size_t)r]; j < crp[(size_t)r + 1]; ++j)
      if (cval[(size_t)j] != 0.f) got.insert({r, cci[(size_t)j]});
  REQUIRE(want == got);  // the values are positive: a sum of duplicates is never zero
  return o;
}

Bytes conv_divide(const Csr& a, int bs, float density) {
  const int n = a.m, mb = (n + bs - 1) / bs;
  const Edge<float> val(a, 1, gen_pos);
  const Block<int> crp((size_t)n + 1), brp((size_t)mb + 1);
  int cnnz = -1, nnzb = -1;
  SUCCEEDS(spmm_divide_nnz(n, a.rp.get(), a.ci.get(), bs, density, crp.get(), brp.get(), &cnnz, &nnzb));
  REQUIRE(crp[(size_t)n] == cnnz && brp[(size_t)mb] == nnzb);
  const Block<int> cci((size_t)cnnz), bci((size_t)nnzb);
  const Block<float> cval((size_t)cnnz), bval((size_t)nnzb * bs * bs);
  SUCCEEDS(spmm_sdivide(n, a.rp.get(), a.ci.get(), val.get(), bs, density, crp.get(), brp.get(), cci.get(),
                        cval.get(), bci.get(), bval.get()));
  Bytes o;
  put(o, crp.get(), crp.size());
  put(o, brp.get(), brp.size());
  put(o, cci.get(), cci.size());
  put(o, cval.get(), cval.size());
  put(o, bci.get(), bci.size());
  put(o, bval.get(), bval.size());
  return o;
}

const Pattern kRect{{3, 0, 0, 9, 1, 0, 4, 4, 4, 0, 0, 2, 17, 1, 1, 0, 5, 6, 0, 0, 1, 1, 2, 3, 5,
                     8, 0, 13, 0, 2, 1, 0, 0, 7, 3, 0, 0},
                    45};  // 37 x 45: no multiple of any block size but 1
Pattern square_of(const Pattern& p) { return {p.len, (int)p.len.size()}; }

void group_convert() {
  for (int bs : {1, 3, 16, 32, 64})
    for (int base : {0, 1}) {
      const Csr a = make_csr(kRect, base, false);
      for (spmm_direction_t dir : {SPMM_DIRECTION_ROW, SPMM_DIRECTION_COLUMN}) {
        g_case = "csr2bsr2csr bs " + std::to_string(bs) + " base " + std::to_string(base);
        conv_csr2bsr(a, a.m, a.k, bs, dir, true);
      }
    }
  ok("convert.csr2bsr2csr");
  g_case = "convert.csr2bsr_empty";
  for (int base : {0, 1}) {
    conv_csr2bsr(make_csr({{}, 5}, base, false), 0, 5, 3, SPMM_DIRECTION_ROW, true);
    conv_csr2bsr(make_csr({{0, 0, 0, 0}, 5}, base, false), 4, 5, 3, SPMM_DIRECTION_ROW, true);
    conv_csr2bsr(make_csr({{0, 0, 0, 0}, 1}, base, false), 4, 0, 3, SPMM_DIRECTION_COLUMN, true);
  }
  ok("convert.csr2bsr_empty");
  g_case = "convert.calculate_nnzb";
  for (int base : {0, 1}) {
    const Csr a = make_csr(square_of(kRect), base, false);
    for (int bs : {1, 3, 16, 32, 64}) {
      const Block<int> brp((size_t)(a.m + bs - 1) / bs + 1);
      int nnzb = -1;
      SUCCEEDS(spmm_xcsr2bsr_nnz(SPMM_DIRECTION_ROW, a.m, a.m, a.rp.get(), a.ci.get(), bs, brp.get(), &nnzb));
      REQUIRE(spmm_calculate_nnzb(a.m, a.rp.get(), a.ci.get(), bs) == nnzb);
    }
    const Csr none = make_csr({{}, 1}, base, false);
    REQUIRE(spmm_calculate_nnzb(0, none.rp.get(), none.ci.get(), 3) == 0);
  }
  ok("convert.calculate_nnzb");
  g_case = "convert.partition_rows";
  for (int base : {0, 1}) {
    const Csr a = make_csr(kRect, base, false);
    for (int nparts : {1, a.m, a.m + 3}) {
      const Block<int> bounds((size_t)nparts + 1);
      SUCCEEDS(spmm_csr_partition_rows(a.m, a.rp.get(), nparts, bounds.get()));
      REQUIRE(bounds[0] == 0 && bounds[(size_t)nparts] == a.m);
      for (int q = 0; q < nparts; ++q) REQUIRE(bounds[(size_t)q] <= bounds[(size_t)q + 1]);
    }
    const Csr none = make_csr({{}, 1}, base, false);
    const Block<int> bounds(3);
    SUCCEEDS(spmm_csr_partition_rows(0, none.rp.get(), 2, bounds.get()));
  }
  ok("convert.partition_rows");
  g_case = "convert.divide";
  for (int base : {0, 1}) {
    const Csr a = make_csr(square_of(kRect), base, false);
    for (int bs : {1, 3, 16, 64})
      for (float density : {0.f, 0.5f, 1.f}) conv_divide(a, bs, density);
    conv_divide(make_csr({{}, 1}, base, false), 3, 0.5f);
    conv_divide(make_csr({{0, 0, 0, 0}, 4}, base, false), 3, 0.f);
  }
  ok("convert.divide");
  g_case = "convert.hybrid_plan";
  for (int base : {0, 1}) {
    const Csr a = make_csr(square_of(kRect), base, false);
    for (int bs : {1, 3, 16, 64}) {
      float density = -1.f;
      int64_t nnzb = -1, rest = -1;
      double est = -1;
      SUCCEEDS(spmm_hybrid_plan(a.m, a.rp.get(), a.ci.get(), bs, 64, 4, 0, 0, &density, &nnzb, &rest, &est));
      REQUIRE(density > 0.f && nnzb >= 0 && rest >= 0 && est >= 0);
      SUCCEEDS(spmm_hybrid_plan(a.m, a.rp.get(), a.ci.get(), bs, 64, 2, 5e12, 6e12, &density, nullptr, nullptr,
                                nullptr));
    }
    const Csr none = make_csr({{}, 1}, base, false);
    float density = -1.f;
    SUCCEEDS(spmm_hybrid_plan(0, none.rp.get(), none.ci.get(), 16, 64, 4, 0, 0, &density, nullptr, nullptr, nullptr));
  }
  ok("convert.hybrid_plan");
}

// ------------------------------------------------------------------ reorder
// which: 0 degree, 1 bfs, 2 rcm (each checked as a permutation), 3 permute_csr with values
// and back through the inverse, 4 block metrics and heat map.
Bytes conv_reorder(const Csr& a, int which) {
  const int n = a.m;
  Bytes o;
  if (which <= 2) {
    const Block<int> perm((size_t)n);
    REQUIRE((which == 0 ? spmm_reorder_degree : which == 1 ? spmm_reorder_bfs : spmm_reorder_rcm)(
                n, a.rp.get(), a.ci.get(), perm.get()) == 0);
    REQUIRE(spmm_check_permutation(n, perm.get()) == 0);
    put(o, perm.get(), perm.size());
  } else if (which == 3) {
    const Block<int> perm((size_t)n), inv((size_t)n);
    REQUIRE(spmm_reorder_rcm(n, a.rp.get(), a.ci.get(), perm.get()) == 0);
    for (int i = 0; i < n; ++i) inv[(size_t)perm[(size_t)i]] = i;
    const Edge<float> val(a, 1, gen_f32);
    const Block<int> rp1((size_t)n + 1), ci1((size_t)a.nnz), rp2((size_t)n + 1), ci2((size_t)a.nnz), ci3((size_t)a.nnz);
    const Block<float> v1((size_t)a.nnz), v2((size_t)a.nnz);
    REQUIRE(spmm_permute_csr(n, a.rp.get(), a.ci.get(), val.get(), perm.get(), rp1.get(), ci1.get(), v1.get()) == 0);
    REQUIRE(spmm_permute_csr(n, rp1.get(), ci1.get(), v1.get(), inv.get(), rp2.get(), ci2.get(), v2.get()) == 0);
    REQUIRE(std::memcmp(rp2.get(), a.rp.get(), sizeof(int) * ((size_t)n + 1)) == 0);
    REQUIRE(a.nnz == 0 || std::memcmp(ci2.get(), a.ci.get(), sizeof(int) * (size_t)a.nnz) == 0);
    REQUIRE(a.nnz == 0 || std::memcmp(v2.get(), val.get(), sizeof(float) * (size_t)a.nnz) == 0);
    REQUIRE(spmm_permute_csr(n, a.rp.get(), a.ci.get(), nullptr, perm.get(), rp2.get(), ci3.get(), nullptr) == 0);
    REQUIRE(a.nnz == 0 || std::memcmp(ci3.get(), ci1.get(), sizeof(int) * (size_t)a.nnz) == 0);
    put(o, rp1.get(), rp1.size());
    put(o, ci1.get(), ci1.size());
    put(o, v1.get(), v1.size());
  } else {
    for (int bs : {1, 3, 16}) {
      spmm_block_metrics_t mt;
      std::memset(&mt, 0, sizeof mt);
      REQUIRE(spmm_block_metrics(n, a.rp.get(), a.ci.get(), bs, &mt) == 0);
      put(o, &mt.nnzb, 1);
      put(o, &mt.density, 1);
      put(o, &mt.utilization, 1);
      put(o, &mt.average, 1);
      if (n > 4096 && bs < 16) continue;  // the heat map is nb * nb ints
      const size_t nb = (size_t)(n + bs - 1) / bs;
      const Block<int> heat(nb * nb);
      REQUIRE(spmm_block_heatmap(n, a.rp.get(), a.ci.get(), bs, heat.get()) == 0);
      int64_t sum = 0;
      for (size_t i = 0; i < heat.size(); ++i) sum += heat[i];
      REQUIRE(sum == a.nnz);
      put(o, heat.get(), heat.size());
    }
  }
  return o;
}

void group_reorder(const std::string& tmp) {
  // two components (0-4 in a ring, 5-8 a star), node 9 isolated; columns sorted
  const Pattern two{{2, 2, 2, 2, 2, 3, 1, 1, 1, 0}, 10};
  Csr g = make_csr(two, 0, false);
  {
    const int cols[] = {1, 4, 0, 2, 1, 3, 2, 4, 0, 3, 6, 7, 8, 5, 5, 5};
    for (size_t i = 0; i < 16; ++i) g.ci[i] = cols[i];
  }
  const Csr sorted = make_csr(square_of(kRect), 0, false, true);
  const Csr none = make_csr({{}, 1}, 0, false);
  static const char* names[] = {"reorder.degree", "reorder.bfs", "reorder.rcm", "reorder.permute_csr",
                                "reorder.metrics_heatmap"};
  for (int which = 0; which < 5; ++which) {
    g_case = names[which];
    conv_reorder(g, which);
    conv_reorder(sorted, which);
    conv_reorder(none, which);
    ok(names[which]);
  }
  g_case = "reorder.files";
  {
    const Block<int> perm(10), again(10);
    REQUIRE(spmm_reorder_bfs(10, g.rp.get(), g.ci.get(), perm.get()) == 0);
    const std::string f = tmp + "/perm.txt";
    REQUIRE(spmm_dump_permutation(f.c_str(), 10, perm.get()) == 0);
    REQUIRE(spmm_load_permutation(f.c_str(), 10, again.get()) == 0);
    REQUIRE(std::memcmp(perm.get(), again.get(), sizeof(int) * 10) == 0);
    again.poison_all();
    REQUIRE(spmm_load_permutation((tmp + "/absent.txt").c_str(), 10, again.get()) == -1);
    const Block<int> longer(11);
    REQUIRE(spmm_load_permutation(f.c_str(), 11, longer.get()) == -1);  // one entry short
    spit(tmp + "/twice.txt", "0 1 1\n");
    const Block<int> three(3);
    REQUIRE(spmm_load_permutation((tmp + "/twice.txt").c_str(), 3, three.get()) == -1);
    REQUIRE(spmm_dump_permutation((tmp + "/empty_perm.txt").c_str(), 0, none.ci.get()) == 0);
    REQUIRE(spmm_load_permutation((tmp + "/empty_perm.txt").c_str(), 0, none.ci.get()) == 0);
    const Block<int> heat(16);
    REQUIRE(spmm_block_heatmap(10, g.rp.get(), g.ci.get(), 3, heat.get()) == 0);
    REQUIRE(spmm_dump_heatmap((tmp + "/heat.txt").c_str(), 4, heat.get()) == 0);
    REQUIRE(slurp(tmp + "/heat.txt").substr(0, 2) == "4\n");
    REQUIRE(spmm_dump_heatmap((tmp + "/heat.txt").c_str(), 0, heat.get()) == -1);
  }
  ok("reorder.files");
}

// ------------------------------------------------------------------ generators
void group_generators() {
  g_case = "gen.random_array";
  {
    const Block<float> x(37), y(37), none(0);
    spmm_host_rng_seed(1234);
    spmm_host_random_array(37, -1.f, 1.f, x.get());
    spmm_host_random_array(0, -1.f, 1.f, none.get());
    spmm_host_rng_seed(1234);
    spmm_host_random_array(37, -1.f, 1.f, y.get());
    REQUIRE(std::memcmp(x.get(), y.get(), sizeof(float) * 37) == 0);
  }
  ok("gen.random_array");
  g_case = "gen.random_csr";
  Bytes first;
  for (int round = 0; round < 2; ++round) {
    Bytes o;
    spmm_host_rng_seed(1234);
    for (const auto& mn : {std::pair<int, int>{13, 29}, {0, 5}, {5, 0}}) {
      const Block<int> rp((size_t)mn.first + 1);
      int* ci = nullptr;
      float* v = nullptr;
      const int64_t nnz = spmm_host_random_csr(mn.first, mn.second, 0.3f, -1.f, 1.f, rp.get(), &ci, &v);
      REQUIRE(nnz >= 0 && rp[(size_t)mn.first] == nnz && ci && v);
      for (int64_t j = 0; j < nnz; ++j) REQUIRE(ci[j] >= 0 && ci[j] < mn.second);
      put(o, rp.get(), rp.size());
      put(o, ci, (size_t)nnz);
      put(o, v, (size_t)nnz);
      spmm_host_free(ci);
      spmm_host_free(v);
    }
    if (round == 0) first = o;
    REQUIRE(o == first);
  }
  ok("gen.random_csr");
  g_case = "gen.random_bsr";
  for (int bs : {1, 3, 16}) {
    const Block<int> rp(8);
    int* ci = nullptr;
    float* v = nullptr;
    const int64_t nnzb = spmm_host_random_bsr(7, 5, bs, 0.4f, -1.f, 1.f, rp.get(), &ci, &v);
    REQUIRE(nnzb >= 0 && rp[7] == nnzb && ci && v);
    float last = v[nnzb ? nnzb * bs * bs - 1 : 0];  // the last value is inside the array
    (void)last;
    spmm_host_free(ci);
    spmm_host_free(v);
  }
  ok("gen.random_bsr");
  g_case = "gen.powerlaw";
  {
    int *rp = nullptr, *ci = nullptr;
    REQUIRE(spmm_host_gen_powerlaw_csr(200, 1500, 60, 2.3, 3, &rp, &ci) == 0);
    REQUIRE(rp[0] == 0 && rp[200] == 1500);
    for (int r = 0; r < 200; ++r)
      for (int j = rp[r]; j < rp[r + 1]; ++j) REQUIRE(ci[j] >= 0 && ci[j] < 200 && (j == rp[r] || ci[j - 1] < ci[j]));
    spmm_host_free(rp);
    spmm_host_free(ci);
    REQUIRE(spmm_host_gen_powerlaw_csr(2, 1, 1, 2.3, 3, &rp, &ci) == 0);
    spmm_host_free(rp);
    spmm_host_free(ci);
    rp = ci = nullptr;
    REQUIRE(spmm_host_gen_powerlaw_csr(0, 0, 1, 2.3, 3, &rp, &ci) == -1 && !rp && !ci);
    REQUIRE(spmm_host_gen_powerlaw_csr(10, 5, 9, 2.3, 3, &rp, &ci) == -1 && !rp && !ci);
  }
  ok("gen.powerlaw");
  g_case = "gen.community";
  {
    int *rp = nullptr, *ci = nullptr;
    int64_t nnz = -1;
    REQUIRE(spmm_host_gen_community_csr(300, 5.0, 4, 30, 0.8, 7, &rp, &ci, &nnz) == 0);
    REQUIRE(rp[0] == 0 && rp[300] == nnz);
    for (int64_t j = 0; j < nnz; ++j) REQUIRE(ci[j] >= 0 && ci[j] < 300);
    spmm_host_free(rp);
    spmm_host_free(ci);
    REQUIRE(spmm_host_gen_community_csr(1, 0.0, 1, 1, 1.0, 7, &rp, &ci, &nnz) == 0 && nnz == 0);
    spmm_host_free(rp);
    spmm_host_free(ci);
    rp = ci = nullptr;
    REQUIRE(spmm_host_gen_community_csr(0, 5.0, 4, 30, 0.8, 7, &rp, &ci, &nnz) == -1 && !rp && !ci);
  }
  ok("gen.community");
}

// ------------------------------------------------------------------ refusals
// Every refusal runs on outputs that are poisoned from end to end: the status must be
// INVALID_VALUE, and "refuses before it writes anything" holds by construction.
void group_refusals() {
  const Pattern pat{{2, 0, 3, 1, 4}, 6};
  const Csr a = make_csr(pat, 0, false);
  const Block<int> rp_dec((size_t)a.m + 1), ci_high((size_t)a.nnz), ci_neg((size_t)a.nnz);
  for (int r = 0; r <= a.m; ++r) rp_dec[(size_t)r] = a.rp[(size_t)r];
  rp_dec[2] = 6;  // 0 2 6 5 6 10
  for (int j = 0; j < a.nnz; ++j) ci_high[(size_t)j] = ci_neg[(size_t)j] = a.ci[(size_t)j];
  ci_high[4] = a.k;
  ci_neg[7] = -1;
  const int n = 5, ld = 8, heads = 2, m = a.m, k = a.k, nnz = a.nnz;
  const spmm_index_base_t b0 = SPMM_INDEX_BASE_ZERO, b1 = SPMM_INDEX_BASE_ONE;
  const spmm_index_base_t b2 = static_cast<spmm_index_base_t>(2);  // what a C caller can pass
  const int* rp = a.rp.get();
  const int* ci = a.ci.get();
  const Dense<float> X(m, heads * n, heads * n + 3, gen_f32), Y(k, heads * n, heads * n + 3, gen_f32);
  const Dense<uint16_t> Xh(m, heads * n, heads * n + 3, gen_f16), Yh(k, heads * n, heads * n + 3, gen_f16);
  const int ldh = heads * n + 3;
  const Edge<float> in(a, heads, gen_pos), in2(a, heads, gen_f32), out(a, heads, gen_f32);
  out.b.poison_all();
  const Dense<float> C(m, heads * n, ldh, gen_f32), dB(k, n, ld, gen_f32);
  const Dense<int> arg(m, n, ld, hash32), arg_in(m, n, ld, hash32);
  C.b.poison_all();
  dB.b.poison_all();
  arg.b.poison_all();
  const float* x = X.get();
  const float* y = Y.get();
  float* o = out.get();

  g_case = "refuse.sddmm";
  {
    auto call = [&](int m_, int n_, int k_, int nnz_, const int* rp_, const int* ci_, spmm_index_base_t b,
                    const float* x_, int ldx, const float* y_, int ldy, float* o_) {
      return spmm_sddmm_csr_host_f32(m_, n_, k_, nnz_, 1.f, rp_, ci_, b, x_, ldx, y_, ldy, 0.f, o_);
    };
    REFUSES(call(-1, n, k, nnz, rp, ci, b0, x, ldh, y, ldh, o));
    REFUSES(call(m, -1, k, nnz, rp, ci, b0, x, ldh, y, ldh, o));
    REFUSES(call(m, n, -1, nnz, rp, ci, b0, x, ldh, y, ldh, o));
    REFUSES(call(m, n, k, -1, rp, ci, b0, x, ldh, y, ldh, o));
    REFUSES(call(m, n, k, nnz, rp, ci, b0, x, n - 1, y, ldh, o));
    REFUSES(call(m, n, k, nnz, rp, ci, b0, x, ldh, y, n - 1, o));
    REFUSES(call(m, n, k, nnz, nullptr, ci, b0, x, ldh, y, ldh, o));
    REFUSES(call(m, n, k, nnz, rp, nullptr, b0, x, ldh, y, ldh, o));
    REFUSES(call(m, n, k, nnz, rp, ci, b0, nullptr, ldh, y, ldh, o));
    REFUSES(call(m, n, k, nnz, rp, ci, b0, x, ldh, nullptr, ldh, o));
    REFUSES(call(m, n, k, nnz, rp, ci, b0, x, ldh, y, ldh, nullptr));
    REFUSES(call(m, n, k, nnz, rp_dec.get(), ci, b0, x, ldh, y, ldh, o));
    REFUSES(call(m, n, k, nnz, rp, ci, b2, x, ldh, y, ldh, o));
    REFUSES(call(m, n, k, nnz, rp, ci, b1, x, ldh, y, ldh, o));      // first entry below the base
    REFUSES(call(m, n, k, nnz - 1, rp, ci, b0, x, ldh, y, ldh, o));  // last entry above nnz
    REFUSES(call(m, n, k, nnz, rp, ci_high.get(), b0, x, ldh, y, ldh, o));
    REFUSES(call(m, n, k, nnz, rp, ci_neg.get(), b0, x, ldh, y, ldh, o));
    REFUSES(call(m, n, k - 1, nnz, rp, ci, b0, x, ldh, y, ldh, o));  // the highest column = k
  }
  ok("refuse.sddmm");

  g_case = "refuse.softmax";
  for (int hd : {0, 1, 2}) {  // 0: the single-head entries
    auto fwd = [&](int m_, int nnz_, int h_, const int* rp_, spmm_index_base_t b, const float* x_, float* y_) {
      return hd ? spmm_edge_softmax_csr_heads_host_f32(m_, nnz_, h_, rp_, b, x_, y_)
                : spmm_edge_softmax_csr_host_f32(m_, nnz_, rp_, b, x_, y_);
    };
    auto bwd = [&](int m_, int nnz_, int h_, const int* rp_, spmm_index_base_t b, const float* y_, const float* g_,
                   float* gx_) {
      return hd ? spmm_edge_softmax_bwd_csr_heads_host_f32(m_, nnz_, h_, rp_, b, y_, g_, gx_)
                : spmm_edge_softmax_bwd_csr_host_f32(m_, nnz_, rp_, b, y_, g_, gx_);
    };
    const float* e = in.get();
    const float* g = in2.get();
    REFUSES(fwd(-1, nnz, hd, rp, b0, e, o));
    REFUSES(fwd(m, -1, hd, rp, b0, e, o));
    REFUSES(fwd(m, nnz, hd, nullptr, b0, e, o));
    REFUSES(fwd(m, nnz, hd, rp, b0, nullptr, o));
    REFUSES(fwd(m, nnz, hd, rp, b0, e, nullptr));
    REFUSES(fwd(m, nnz, hd, rp_dec.get(), b0, e, o));
    REFUSES(fwd(m, nnz, hd, rp, b2, e, o));
    REFUSES(fwd(m, nnz, hd, rp, b1, e, o));
    REFUSES(fwd(m, nnz - 1, hd, rp, b0, e, o));
    REFUSES(bwd(-1, nnz, hd, rp, b0, e, g, o));
    REFUSES(bwd(m, -1, hd, rp, b0, e, g, o));
    REFUSES(bwd(m, nnz, hd, nullptr, b0, e, g, o));
    REFUSES(bwd(m, nnz, hd, rp, b0, nullptr, g, o));
    REFUSES(bwd(m, nnz, hd, rp, b0, e, nullptr, o));
    REFUSES(bwd(m, nnz, hd, rp, b0, e, g, nullptr));
    REFUSES(bwd(m, nnz, hd, rp_dec.get(), b0, e, g, o));
    REFUSES(bwd(m, nnz, hd, rp, b2, e, g, o));
    REFUSES(bwd(m, nnz, hd, rp, b1, e, g, o));
    REFUSES(bwd(m, nnz - 1, hd, rp, b0, e, g, o));
    if (hd) {
      REFUSES(fwd(m, nnz, 0, rp, b0, e, o));
      REFUSES(bwd(m, nnz, -1, rp, b0, e, g, o));
    }
  }
  ok("refuse.softmax");

  g_case = "refuse.sddmm_heads";
  for (int type = 0; type < 3; ++type) {  // f32, f16, bf16
    auto call = [&](int m_, int d_, int k_, int nnz_, int h_, const int* rp_, const int* ci_, spmm_index_base_t b,
                    bool xnull, int ldx, bool ynull, int ldy, float* o_) {
      if (type == 0)
        return spmm_sddmm_csr_heads_host_f32(m_, d_, k_, nnz_, h_, 1.f, rp_, ci_, b, xnull ? nullptr : x, ldx,
                                             ynull ? nullptr : y, ldy, 0.f, o_);
      return (type == 1 ? spmm_sddmm_csr_heads_host_f16 : spmm_sddmm_csr_heads_host_bf16)(
          m_, d_, k_, nnz_, h_, 1.f, rp_, ci_, b, xnull ? nullptr : Xh.get(), ldx, ynull ? nullptr : Yh.get(), ldy,
          0.f, o_);
    };
    REFUSES(call(-1, n, k, nnz, heads, rp, ci, b0, false, ldh, false, ldh, o));
    REFUSES(call(m, -1, k, nnz, heads, rp, ci, b0, false, ldh, false, ldh, o));
    REFUSES(call(m, n, -1, nnz, heads, rp, ci, b0, false, ldh, false, ldh, o));
    REFUSES(call(m, n, k, -1, heads, rp, ci, b0, false, ldh, false, ldh, o));
    REFUSES(call(m, n, k, nnz, 0, rp, ci, b0, false, ldh, false, ldh, o));
    REFUSES(call(m, n, k, nnz, heads, rp, ci, b0, false, heads * n - 1, false, ldh, o));
    REFUSES(call(m, n, k, nnz, heads, rp, ci, b0, false, ldh, false, heads * n - 1, o));
    REFUSES(call(m, n, k, nnz, heads, nullptr, ci, b0, false, ldh, false, ldh, o));
    REFUSES(call(m, n, k, nnz, heads, rp, nullptr, b0, false, ldh, false, ldh, o));
    REFUSES(call(m, n, k, nnz, heads, rp, ci, b0, true, ldh, false, ldh, o));
    REFUSES(call(m, n, k, nnz, heads, rp, ci, b0, false, ldh, true, ldh, o));
    REFUSES(call(m, n, k, nnz, heads, rp, ci, b0, false, ldh, false, ldh, nullptr));
    REFUSES(call(m, n, k, nnz, heads, rp_dec.get(), ci, b0, false, ldh, false, ldh, o));
    REFUSES(call(m, n, k, nnz, heads, rp, ci, b2, false, ldh, false, ldh, o));
    REFUSES(call(m, n, k, nnz, heads, rp, ci, b1, false, ldh, false, ldh, o));
    REFUSES(call(m, n, k, nnz - 1, heads, rp, ci, b0, false, ldh, false, ldh, o));
    REFUSES(call(m, n, k, nnz, heads, rp, ci_high.get(), b0, false, ldh, false, ldh, o));
    REFUSES(call(m, n, k, nnz, heads, rp, ci_neg.get(), b0, false, ldh, false, ldh, o));
  }
  ok("refuse.sddmm_heads");

  g_case = "refuse.csrmm_heads";
  for (int type = 0; type < 3; ++type) {
    auto call = [&](int m_, int d_, int k_, int nnz_, int h_, const int* rp_, const int* ci_, const float* v_,
                    spmm_index_base_t b, bool bnull, int ldb, float* c_, int ldc) {
      if (type == 0)
        return spmm_csrmm_heads_host_f32(m_, d_, k_, nnz_, h_, 1.f, rp_, ci_, v_, b, bnull ? nullptr : y, ldb, 0.f,
                                         c_, ldc);
      return (type == 1 ? spmm_csrmm_heads_host_f16 : spmm_csrmm_heads_host_bf16)(
          m_, d_, k_, nnz_, h_, 1.f, rp_, ci_, v_, b, bnull ? nullptr : Yh.get(), ldb, 0.f, c_, ldc);
    };
    const float* v = in.get();
    float* c = C.get();
    REFUSES(call(-1, n, k, nnz, heads, rp, ci, v, b0, false, ldh, c, ldh));
    REFUSES(call(m, -1, k, nnz, heads, rp, ci, v, b0, false, ldh, c, ldh));
    REFUSES(call(m, n, -1, nnz, heads, rp, ci, v, b0, false, ldh, c, ldh));
    REFUSES(call(m, n, k, -1, heads, rp, ci, v, b0, false, ldh, c, ldh));
    REFUSES(call(m, n, k, nnz, 0, rp, ci, v, b0, false, ldh, c, ldh));
    REFUSES(call(m, n, k, nnz, heads, nullptr, ci, v, b0, false, ldh, c, ldh));
    REFUSES(call(m, n, k, nnz, heads, rp, nullptr, v, b0, false, ldh, c, ldh));
    REFUSES(call(m, n, k, nnz, heads, rp, ci, nullptr, b0, false, ldh, c, ldh));
    REFUSES(call(m, n, k, nnz, heads, rp, ci, v, b0, true, ldh, c, ldh));
    REFUSES(call(m, n, k, nnz, heads, rp, ci, v, b0, false, ldh, nullptr, ldh));
    REFUSES(call(m, n, k, nnz, heads, rp, ci, v, b0, false, heads * n - 1, c, ldh));
    REFUSES(call(m, n, k, nnz, heads, rp, ci, v, b0, false, ldh, c, heads * n - 1));
    REFUSES(call(m, n, k, nnz, heads, rp_dec.get(), ci, v, b0, false, ldh, c, ldh));
    REFUSES(call(m, n, k, nnz, heads, rp, ci, v, b2, false, ldh, c, ldh));
    REFUSES(call(m, n, k, nnz, heads, rp, ci, v, b1, false, ldh, c, ldh));
    REFUSES(call(m, n, k, nnz - 1, heads, rp, ci, v, b0, false, ldh, c, ldh));
    REFUSES(call(m, n, k, nnz, heads, rp, ci_high.get(), v, b0, false, ldh, c, ldh));
    REFUSES(call(m, n, k, nnz, heads, rp, ci_neg.get(), v, b0, false, ldh, c, ldh));
  }
  ok("refuse.csrmm_heads");

  g_case = "refuse.reduce_fwd";
  {
    const Dense<float> B(k, n, ld, gen_f32), Cr(m, n, ld, gen_f32);
    Cr.b.poison_all();
    auto call = [&](int op, int m_, int n_, int k_, int nnz_, const int* rp_, const int* ci_, spmm_index_base_t b,
                    const float* b_, int ldb, float* c_, int ldc, int* arg_, int ldarg) {
      return spmm_csrmm_reduce_host_f32(op ? SPMM_REDUCE_MIN : SPMM_REDUCE_MAX, m_, n_, k_, nnz_, rp_, ci_,
                                        in.get(), b, b_, ldb, c_, ldc, arg_, ldarg);
    };
    const float* bb = B.get();
    float* c = Cr.get();
    int* w = arg.get();
    REFUSES(call(0, -1, n, k, nnz, rp, ci, b0, bb, ld, c, ld, w, ld));
    REFUSES(call(0, m, -1, k, nnz, rp, ci, b0, bb, ld, c, ld, w, ld));
    REFUSES(call(1, m, n, -1, nnz, rp, ci, b0, bb, ld, c, ld, w, ld));
    REFUSES(call(1, m, n, k, -1, rp, ci, b0, bb, ld, c, ld, w, ld));
    REFUSES(call(0, m, n, k, nnz, nullptr, ci, b0, bb, ld, c, ld, w, ld));
    REFUSES(call(0, m, n, k, nnz, rp, nullptr, b0, bb, ld, c, ld, w, ld));
    REFUSES(call(0, m, n, k, nnz, rp, ci, b0, nullptr, ld, c, ld, w, ld));
    REFUSES(call(0, m, n, k, nnz, rp, ci, b0, bb, ld, nullptr, ld, w, ld));
    REFUSES(call(0, m, n, k, nnz, rp, ci, b0, bb, n - 1, c, ld, w, ld));
    REFUSES(call(0, m, n, k, nnz, rp, ci, b0, bb, ld, c, n - 1, w, ld));
    REFUSES(call(0, m, n, k, nnz, rp, ci, b0, bb, ld, c, ld, w, n - 1));
    REFUSES(call(0, m, n, k, nnz, rp_dec.get(), ci, b0, bb, ld, c, ld, w, ld));
    REFUSES(call(0, m, n, k, nnz, rp, ci, b2, bb, ld, c, ld, w, ld));
    REFUSES(spmm_csrmm_reduce_host_f32(static_cast<spmm_reduce_t>(2), m, n, k, nnz, rp, ci, in.get(), b0, bb, ld,
                                       c, ld, w, ld));
    REFUSES(call(0, m, n, k, nnz, rp, ci, b1, bb, ld, c, ld, w, ld));
    REFUSES(call(0, m, n, k, nnz - 1, rp, ci, b0, bb, ld, c, ld, w, ld));
    REFUSES(call(1, m, n, k, nnz, rp, ci_high.get(), b0, bb, ld, c, ld, w, ld));
    REFUSES(call(1, m, n, k, nnz, rp, ci_neg.get(), b0, bb, ld, c, ld, w, ld));
  }
  ok("refuse.reduce_fwd");

  g_case = "refuse.reduce_bwd";
  {
    const Block<int> trp((size_t)k + 1), tci((size_t)nnz), perm((size_t)nnz), trp_dec((size_t)k + 1);
    const Block<int> tci_high((size_t)nnz), perm_high((size_t)nnz), perm_neg((size_t)nnz);
    SUCCEEDS(spmm_csr2csc(m, k, nnz, nullptr, rp, ci, 0, b0, b0, nullptr, trp.get(), tci.get(), perm.get()));
    for (int r = 0; r <= k; ++r) trp_dec[(size_t)r] = trp[(size_t)r];
    REQUIRE(trp[2] >= 1);
    trp_dec[1] = trp[2] + 1;  // a decrease from row 1 to row 2, both ends unchanged
    REQUIRE(trp_dec[1] <= nnz);
    for (int j = 0; j < nnz; ++j) {
      tci_high[(size_t)j] = tci[(size_t)j];
      perm_high[(size_t)j] = perm_neg[(size_t)j] = perm[(size_t)j];
    }
    tci_high[3] = m;
    perm_high[2] = nnz;
    perm_neg[5] = -1;
    const Dense<float> dC(m, n, ld, gen_f32);
    auto call = [&](int k_, int n_, int m_, int nnz_, const int* trp_, const int* tci_, const int* perm_,
                    spmm_index_base_t b, const float* dc_, int lddc, const int* arg_, int ldarg, float* db_,
                    int lddb) {
      return spmm_csrmm_reduce_bwd_host_f32(k_, n_, m_, nnz_, trp_, tci_, perm_, in.get(), b, dc_, lddc, arg_,
                                            ldarg, db_, lddb);
    };
    const int* t0 = trp.get();
    const int* t1 = tci.get();
    const int* pm = perm.get();
    const float* dc = dC.get();
    const int* ai = arg_in.get();
    float* db = dB.get();
    REFUSES(call(-1, n, m, nnz, t0, t1, pm, b0, dc, ld, ai, ld, db, ld));
    REFUSES(call(k, -1, m, nnz, t0, t1, pm, b0, dc, ld, ai, ld, db, ld));
    REFUSES(call(k, n, -1, nnz, t0, t1, pm, b0, dc, ld, ai, ld, db, ld));
    REFUSES(call(k, n, m, -1, t0, t1, pm, b0, dc, ld, ai, ld, db, ld));
    REFUSES(call(k, n, m, nnz, nullptr, t1, pm, b0, dc, ld, ai, ld, db, ld));
    REFUSES(call(k, n, m, nnz, t0, nullptr, pm, b0, dc, ld, ai, ld, db, ld));
    REFUSES(call(k, n, m, nnz, t0, t1, nullptr, b0, dc, ld, ai, ld, db, ld));
    REFUSES(call(k, n, m, nnz, t0, t1, pm, b0, nullptr, ld, ai, ld, db, ld));
    REFUSES(call(k, n, m, nnz, t0, t1, pm, b0, dc, ld, nullptr, ld, db, ld));
    REFUSES(call(k, n, m, nnz, t0, t1, pm, b0, dc, ld, ai, ld, nullptr, ld));
    REFUSES(call(k, n, m, nnz, t0, t1, pm, b0, dc, n - 1, ai, ld, db, ld));
    REFUSES(call(k, n, m, nnz, t0, t1, pm, b0, dc, ld, ai, n - 1, db, ld));
    REFUSES(call(k, n, m, nnz, t0, t1, pm, b0, dc, ld, ai, ld, db, n - 1));
    REFUSES(call(k, n, m, nnz, trp_dec.get(), t1, pm, b0, dc, ld, ai, ld, db, ld));
    REFUSES(call(k, n, m, nnz, t0, t1, pm, b2, dc, ld, ai, ld, db, ld));
    REFUSES(call(k, n, m, nnz, t0, t1, pm, b1, dc, ld, ai, ld, db, ld));
    REFUSES(call(k, n, m, nnz - 1, t0, t1, pm, b0, dc, ld, ai, ld, db, ld));
    REFUSES(call(k, n, m, nnz, t0, tci_high.get(), pm, b0, dc, ld, ai, ld, db, ld));
    REFUSES(call(k, n, m, nnz, t0, t1, perm_high.get(), b0, dc, ld, ai, ld, db, ld));
    REFUSES(call(k, n, m, nnz, t0, t1, perm_neg.get(), b0, dc, ld, ai, ld, db, ld));
  }
  ok("refuse.reduce_bwd");

  g_case = "refuse.csr2csc";
  {
    const Block<int> tcp((size_t)k + 1), tri((size_t)nnz), perm((size_t)nnz);
    const Block<float> tv((size_t)nnz);
    tcp.poison_all();
    tri.poison_all();
    perm.poison_all();
    tv.poison_all();
    auto call = [&](int m_, int n_, int nnz_, const float* v_, const int* rp_, const int* ci_, int vb,
                    spmm_index_base_t ba, float* tv_, int* tcp_, int* tri_) {
      return spmm_csr2csc(m_, n_, nnz_, v_, rp_, ci_, vb, ba, b0, tv_, tcp_, tri_, perm.get());
    };
    const float* v = in2.get();
    REFUSES(call(-1, k, nnz, v, rp, ci, 4, b0, tv.get(), tcp.get(), tri.get()));
    REFUSES(call(m, -1, nnz, v, rp, ci, 4, b0, tv.get(), tcp.get(), tri.get()));
    REFUSES(call(m, k, -1, v, rp, ci, 4, b0, tv.get(), tcp.get(), tri.get()));
    REFUSES(call(m, k, nnz, v, rp, ci, 3, b0, tv.get(), tcp.get(), tri.get()));
    REFUSES(call(m, k, nnz, v, nullptr, ci, 4, b0, tv.get(), tcp.get(), tri.get()));
    REFUSES(call(m, k, nnz, v, rp, nullptr, 4, b0, tv.get(), tcp.get(), tri.get()));
    REFUSES(call(m, k, nnz, nullptr, rp, ci, 4, b0, tv.get(), tcp.get(), tri.get()));
    REFUSES(call(m, k, nnz, v, rp, ci, 4, b0, nullptr, tcp.get(), tri.get()));
    REFUSES(call(m, k, nnz, v, rp, ci, 4, b0, tv.get(), nullptr, tri.get()));
    REFUSES(call(m, k, nnz, v, rp, ci, 4, b0, tv.get(), tcp.get(), nullptr));
    REFUSES(call(m, k, nnz, v, rp_dec.get(), ci, 4, b0, tv.get(), tcp.get(), tri.get()));
    REFUSES(call(m, k, nnz, v, rp, ci, 4, b2, tv.get(), tcp.get(), tri.get()));
    REFUSES(spmm_csr2csc(m, k, nnz, v, rp, ci, 4, b0, b2, tv.get(), tcp.get(), tri.get(), perm.get()));
    REFUSES(call(m, k, nnz, v, rp, ci, 4, b1, tv.get(), tcp.get(), tri.get()));      // below baseA
    REFUSES(call(m, k, nnz - 1, v, rp, ci, 4, b0, tv.get(), tcp.get(), tri.get()));  // not the pointer's nnz
    REFUSES(call(m, k, nnz + 1, v, rp, ci, 4, b0, tv.get(), tcp.get(), tri.get()));
    REFUSES(call(m, k, nnz, v, rp, ci_high.get(), 4, b0, tv.get(), tcp.get(), tri.get()));
    REFUSES(call(m, k, nnz, v, rp, ci_neg.get(), 4, b0, tv.get(), tcp.get(), tri.get()));
  }
  ok("refuse.csr2csc");

  g_case = "refuse.reorder";
  {
    const Csr sq = make_csr(square_of(pat), 0, false);  // 5 x 5
    const Block<int> p5(5), id(5), twice(5), rp2(6), ci2((size_t)sq.nnz), sq_high((size_t)sq.nnz);
    p5.poison_all();
    rp2.poison_all();
    ci2.poison_all();
    for (int i = 0; i < 5; ++i) id[(size_t)i] = twice[(size_t)i] = i;
    twice[3] = 2;
    for (int j = 0; j < sq.nnz; ++j) sq_high[(size_t)j] = sq.ci[(size_t)j];
    sq_high[1] = 5;
    for (auto f : {spmm_reorder_degree, spmm_reorder_bfs, spmm_reorder_rcm}) {
      REQUIRE(f(-1, sq.rp.get(), sq.ci.get(), p5.get()) == -1);
      REQUIRE(f(5, nullptr, sq.ci.get(), p5.get()) == -1);
      REQUIRE(f(5, sq.rp.get(), nullptr, p5.get()) == -1);
      REQUIRE(f(5, sq.rp.get(), sq.ci.get(), nullptr) == -1);
      REQUIRE(f(5, rp_dec.get(), sq.ci.get(), p5.get()) == -1);
      REQUIRE(f(5, sq.rp.get(), sq_high.get(), p5.get()) == -1);
      REQUIRE(f(5, sq.rp.get(), ci_neg.get(), p5.get()) == -1);
    }
    REQUIRE(spmm_check_permutation(5, twice.get()) == -1);
    REQUIRE(spmm_check_permutation(-1, id.get()) == -1);
    REQUIRE(spmm_check_permutation(5, nullptr) == -1);
    REQUIRE(spmm_permute_csr(5, sq.rp.get(), sq.ci.get(), nullptr, twice.get(), rp2.get(), ci2.get(), nullptr) == -1);
    REQUIRE(spmm_permute_csr(5, sq.rp.get(), sq_high.get(), nullptr, id.get(), rp2.get(), ci2.get(), nullptr) == -1);
    REQUIRE(spmm_permute_csr(5, sq.rp.get(), sq.ci.get(), nullptr, id.get(), nullptr, ci2.get(), nullptr) == -1);
    REQUIRE(spmm_permute_csr(5, sq.rp.get(), sq.ci.get(), nullptr, id.get(), rp2.get(), nullptr, nullptr) == -1);
    REQUIRE(spmm_permute_csr(5, sq.rp.get(), sq.ci.get(), in2.get(), id.get(), rp2.get(), ci2.get(), nullptr) == -1);
    spmm_block_metrics_t mt;
    REQUIRE(spmm_block_metrics(5, sq.rp.get(), sq.ci.get(), 0, &mt) == -1);
    REQUIRE(spmm_block_metrics(5, sq.rp.get(), sq.ci.get(), 2, nullptr) == -1);
    REQUIRE(spmm_block_metrics(5, sq.rp.get(), sq_high.get(), 2, &mt) == -1);
    REQUIRE(spmm_block_heatmap(5, sq.rp.get(), sq.ci.get(), 2, nullptr) == -1);
    REQUIRE(spmm_block_heatmap(5, sq.rp.get(), sq_high.get(), 2, ci2.get()) == -1);
  }
  ok("refuse.reorder");
}

// ------------------------------------------------------------------ loaders
struct Loaded {
  int* rp = reinterpret_cast<int*>(0x10);  // sentinels: a refusal leaves the out-pointers alone
  int* ci = reinterpret_cast<int*>(0x20);
  float* val = reinterpret_cast<float*>(0x30);
  int n = -7;
  int64_t nnz = -7;
  bool untouched() const {
    return rp == reinterpret_cast<int*>(0x10) && ci == reinterpret_cast<int*>(0x20) &&
           val == reinterpret_cast<float*>(0x30) && n == -7 && nnz == -7;
  }
  void release() {
    spmm_host_free(rp);
    spmm_host_free(ci);
    if (val != reinterpret_cast<float*>(0x30)) spmm_host_free(val);
    *this = Loaded();
  }
};

void refuse_graph(const std::string& tmp, const char* what, const std::string& text) {
  g_case = std::string("loaders.malformed graph: ") + what;
  spit(tmp + "/bad_graph.txt", text);
  Loaded l;
  REQUIRE(spmm_host_load_graph((tmp + "/bad_graph.txt").c_str(), &l.rp, &l.ci, &l.n, &l.nnz) == -1);
  REQUIRE(l.untouched());
}

void refuse_csr(const std::string& tmp, const char* what, const std::string& indptr, const std::string& indices) {
  g_case = std::string("loaders.malformed csr: ") + what;
  spit(tmp + "/bad_indptr.txt", indptr);
  spit(tmp + "/bad_indices.txt", indices);
  std::remove((tmp + "/bad.csrbin").c_str());
  Loaded l;
  REQUIRE(spmm_host_load_csr((tmp + "/bad").c_str(), &l.rp, &l.ci, &l.n, &l.nnz) == -1);
  REQUIRE(l.untouched());
  REQUIRE(spmm_host_load_csr_cached((tmp + "/bad").c_str(), &l.rp, &l.ci, &l.n, &l.nnz) == -1);
  REQUIRE(l.untouched());
  struct stat st;
  REQUIRE(stat((tmp + "/bad.csrbin").c_str(), &st) != 0);  // nothing refused is cached
}

void refuse_bin(const std::string& tmp, const char* what, const std::string& bytes, int status) {
  g_case = std::string("loaders.malformed csrbin: ") + what;
  spit(tmp + "/bad.csrbin", bytes);
  Loaded l;
  REQUIRE(spmm_host_load_csr_bin((tmp + "/bad.csrbin").c_str(), &l.rp, &l.ci, &l.val, &l.n, &l.nnz) == status);
  REQUIRE(l.untouched());
}

void group_loaders(const std::string& tmp) {
  const Csr a = make_csr(kRect, 0, false, true);
  const Edge<float> val(a, 1, gen_f32);
  auto same = [&](const Loaded& l) {
    return l.n == a.m && l.nnz == a.nnz && std::memcmp(l.rp, a.rp.get(), sizeof(int) * ((size_t)a.m + 1)) == 0 &&
           std::memcmp(l.ci, a.ci.get(), sizeof(int) * (size_t)a.nnz) == 0;
  };
  g_case = "loaders.text_round_trip";
  {
    Loaded l;
    REQUIRE(spmm_host_dump_csr((tmp + "/g").c_str(), a.m, a.nnz, a.rp.get(), a.ci.get()) == 0);
    REQUIRE(spmm_host_load_csr((tmp + "/g").c_str(), &l.rp, &l.ci, &l.n, &l.nnz) == 0 && same(l));
    l.release();
    const Csr none = make_csr({{}, 1}, 0, false);
    REQUIRE(spmm_host_dump_csr((tmp + "/none").c_str(), 0, 0, none.rp.get(), nullptr) == 0);
    REQUIRE(spmm_host_load_csr((tmp + "/none").c_str(), &l.rp, &l.ci, &l.n, &l.nnz) == 0 && l.n == 0 && l.nnz == 0);
    l.release();
  }
  ok("loaders.text_round_trip");
  g_case = "loaders.edge_list";
  {
    Loaded l;
    spit(tmp + "/edges.txt", "4 5\n2 3\n0 1\n2 0\n0 1\n3 3\n");
    REQUIRE(spmm_host_load_graph((tmp + "/edges.txt").c_str(), &l.rp, &l.ci, &l.n, &l.nnz) == 0);
    const int rp[] = {0, 2, 2, 4, 5}, ci[] = {1, 1, 0, 3, 3};
    REQUIRE(l.n == 4 && l.nnz == 5 && std::memcmp(l.rp, rp, sizeof rp) == 0 && std::memcmp(l.ci, ci, sizeof ci) == 0);
    l.release();
    spit(tmp + "/no_edges.txt", "3 0\n");
    REQUIRE(spmm_host_load_graph((tmp + "/no_edges.txt").c_str(), &l.rp, &l.ci, &l.n, &l.nnz) == 0);
    REQUIRE(l.n == 3 && l.nnz == 0 && l.rp[3] == 0);
    l.release();
  }
  ok("loaders.edge_list");
  g_case = "loaders.binary_round_trip";
  for (int with_val = 0; with_val < 2; ++with_val) {
    const std::string f = tmp + "/g.csrbin";
    Loaded l;
    REQUIRE(spmm_host_save_csr_bin(f.c_str(), a.m, a.nnz, a.rp.get(), a.ci.get(), with_val ? val.get() : nullptr) == 0);
    REQUIRE(spmm_host_load_csr_bin(f.c_str(), &l.rp, &l.ci, &l.val, &l.n, &l.nnz) == 0 && same(l));
    REQUIRE(with_val ? std::memcmp(l.val, val.get(), sizeof(float) * (size_t)a.nnz) == 0 : l.val == nullptr);
    if (!with_val) l.val = Loaded().val;
    l.release();
    REQUIRE(spmm_host_load_csr_bin(f.c_str(), &l.rp, &l.ci, nullptr, &l.n, &l.nnz) == 0 && same(l));
    l.release();
  }
  ok("loaders.binary_round_trip");
  g_case = "loaders.cached";
  {
    const std::string prefix = tmp + "/c", bin = prefix + ".csrbin";
    Loaded l;
    REQUIRE(spmm_host_dump_csr(prefix.c_str(), a.m, a.nnz, a.rp.get(), a.ci.get()) == 0);
    REQUIRE(spmm_host_load_csr_cached(prefix.c_str(), &l.rp, &l.ci, &l.n, &l.nnz) == 0 && same(l));  // parses
    l.release();
    const std::string cache = slurp(bin);
    REQUIRE(!cache.empty());
    std::remove((prefix + "_indices.txt").c_str());  // only the cache can serve this one
    REQUIRE(spmm_host_load_csr_cached(prefix.c_str(), &l.rp, &l.ci, &l.n, &l.nnz) == 0 && same(l));
    l.release();
    REQUIRE(spmm_host_dump_csr(prefix.c_str(), a.m, a.nnz, a.rp.get(), a.ci.get()) == 0);
    std::string corrupt = cache;
    corrupt[corrupt.size() - 5] ^= 1;
    spit(bin, corrupt);  // newer than the text, and corrupt: the text is parsed, the cache rewritten
    REQUIRE(spmm_host_load_csr_cached(prefix.c_str(), &l.rp, &l.ci, &l.n, &l.nnz) == 0 && same(l));
    l.release();
    REQUIRE(slurp(bin) == cache);
  }
  ok("loaders.cached");

  refuse_graph(tmp, "empty file", "");
  refuse_graph(tmp, "one token", "3\n");
  refuse_graph(tmp, "non-numeric header", "x 2\n0 1\n1 2\n");
  refuse_graph(tmp, "non-numeric edge", "3 2\n0 1\n1 y\n");
  refuse_graph(tmp, "token past int range", "3 2\n0 1\n1 4294967297\n");
  refuse_graph(tmp, "header past long long", "99999999999999999999 2\n0 1\n1 2\n");
  refuse_graph(tmp, "fewer tokens than the header says", "3 3\n0 1\n1 2\n");
  refuse_graph(tmp, "odd token count", "3 2\n0 1\n1\n");
  refuse_graph(tmp, "destination out of range", "3 2\n0 1\n1 7\n");
  refuse_graph(tmp, "negative destination", "3 1\n0 -4\n");
  refuse_graph(tmp, "destination = n", "3 1\n0 3\n");
  refuse_graph(tmp, "source out of range", "3 2\n0 1\n5 0\n");
  refuse_graph(tmp, "negative source", "3 1\n-1 0\n");
  refuse_graph(tmp, "nnz of 2e9 over two edges", "3 2000000000\n0 1\n1 2\n");
  refuse_graph(tmp, "nnz past int range", "3 4294967296\n0 1\n");
  refuse_graph(tmp, "negative n", "-3 1\n0 1\n");
  refuse_graph(tmp, "negative nnz", "3 -1\n0 1\n");
  ok("loaders.malformed_graph");

  refuse_csr(tmp, "empty files", "", "");
  refuse_csr(tmp, "one token", "3\n", "1\n");
  refuse_csr(tmp, "non-numeric row pointer", "3\n0 1 x\n", "1\n0\n");
  refuse_csr(tmp, "non-numeric column", "3\n0 1 1\n", "1\nz\n");
  refuse_csr(tmp, "token past int range", "3\n0 1 1\n", "1\n4294967297\n");
  refuse_csr(tmp, "one row pointer short", "4\n0 1 1\n", "1\n0\n");
  refuse_csr(tmp, "one column short", "3\n0 1 2\n", "2\n0\n");
  refuse_csr(tmp, "decreasing row pointer", "3\n0 5 1\n", "1\n9\n");
  refuse_csr(tmp, "row pointer not from 0", "3\n1 1 2\n", "2\n0 1\n");
  refuse_csr(tmp, "last row pointer is not nnz", "3\n0 1 1\n", "2\n0 1\n");
  refuse_csr(tmp, "negative column", "3\n0 1 2\n", "2\n0 -1\n");
  refuse_csr(tmp, "indptr count of 0", "0\n", "0\n");
  refuse_csr(tmp, "negative indptr count", "-2\n0\n", "0\n");
  refuse_csr(tmp, "negative nnz", "2\n0 0\n", "-1\n");
  refuse_csr(tmp, "nnz of 2e9 over one column", "2\n0 1\n", "2000000000\n0\n");
  refuse_csr(tmp, "indptr count of 2e9", "2000000000\n0 1\n", "1\n0\n");
  ok("loaders.malformed_csr");

  {
    REQUIRE(spmm_host_save_csr_bin((tmp + "/v.csrbin").c_str(), a.m, a.nnz, a.rp.get(), a.ci.get(), val.get()) == 0);
    const std::string good = slurp(tmp + "/v.csrbin");
    const size_t head = good.size() - 4 * ((size_t)a.m + 1) - 8 * (size_t)a.nnz;
    REQUIRE(head == 56);
    refuse_bin(tmp, "empty", "", -1);
    refuse_bin(tmp, "not a cache", "not a cache", -1);
    refuse_bin(tmp, "truncated header", good.substr(0, head - 3), -1);
    refuse_bin(tmp, "truncated inside rowptr", good.substr(0, head + 4 * 5 + 1), -1);
    refuse_bin(tmp, "truncated inside colind", good.substr(0, head + 4 * ((size_t)a.m + 1) + 4 * 7 + 2), -1);
    refuse_bin(tmp, "truncated inside val", good.substr(0, good.size() - 6), -1);
    std::string bad = good;
    bad[good.size() / 2] ^= 0x10;
    refuse_bin(tmp, "one bit flipped", bad, -2);
    const int64_t far = (int64_t)1 << 30;
    bad = good;
    std::memcpy(&bad[16], &far, 8);  // n far past the file's size
    refuse_bin(tmp, "n far past the file", bad, -1);
    bad = good;
    std::memcpy(&bad[24], &far, 8);  // nnz far past the file's size
    refuse_bin(tmp, "nnz far past the file", bad, -1);
    const int64_t neg = -1;
    bad = good;
    std::memcpy(&bad[16], &neg, 8);
    refuse_bin(tmp, "negative n", bad, -1);
    // arrays that are intact by their checksums and still no CSR: written by the library
    const int rp_bad[] = {0, 5, 1}, ci_bad[] = {9}, rp_ok[] = {0, 1, 2}, ci_neg[] = {0, -1};
    REQUIRE(spmm_host_save_csr_bin((tmp + "/w.csrbin").c_str(), 2, 1, rp_bad, ci_bad, nullptr) == 0);
    refuse_bin(tmp, "decreasing row pointer", slurp(tmp + "/w.csrbin"), -1);
    REQUIRE(spmm_host_save_csr_bin((tmp + "/w.csrbin").c_str(), 2, 2, rp_ok, ci_neg, nullptr) == 0);
    refuse_bin(tmp, "negative column", slurp(tmp + "/w.csrbin"), -1);
    REQUIRE(spmm_host_save_csr_bin((tmp + "/w.csrbin").c_str(), 2, 1, rp_ok, ci_bad, nullptr) == 0);
    refuse_bin(tmp, "last row pointer is not nnz", slurp(tmp + "/w.csrbin"), -1);
  }
  ok("loaders.malformed_csrbin");

  g_case = "loaders.arguments";
  {
    Loaded l;
    REQUIRE(spmm_host_load_graph(nullptr, &l.rp, &l.ci, &l.n, &l.nnz) == -1);
    REQUIRE(spmm_host_load_graph((tmp + "/absent.txt").c_str(), &l.rp, &l.ci, &l.n, &l.nnz) == -1);
    REQUIRE(spmm_host_load_csr((tmp + "/absent").c_str(), &l.rp, &l.ci, &l.n, &l.nnz) == -1);
    REQUIRE(spmm_host_load_csr_cached((tmp + "/absent").c_str(), &l.rp, &l.ci, &l.n, &l.nnz) == -1);
    REQUIRE(spmm_host_load_csr_bin((tmp + "/absent.csrbin").c_str(), &l.rp, &l.ci, &l.val, &l.n, &l.nnz) == -1);
    REQUIRE(spmm_host_load_csr((tmp + "/g").c_str(), nullptr, &l.ci, &l.n, &l.nnz) == -1);
    REQUIRE(spmm_host_dump_csr((tmp + "/no/such/dir/g").c_str(), a.m, a.nnz, a.rp.get(), a.ci.get()) == -1);
    REQUIRE(spmm_host_save_csr_bin((tmp + "/no/such/dir/g.csrbin").c_str(), a.m, a.nnz, a.rp.get(), a.ci.get(), nullptr) == -1);
    REQUIRE(l.untouched());
  }
  ok("loaders.arguments");
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) {
    std::fprintf(stderr, "usage: host_sanitize forms|convert|reorder|generators|threads|refusals|loaders <tmpdir>\n");
    return 2;
  }
  const std::string group = argv[1], tmp = argv[2];
  g_case = "setup";
  check_setup();
  if (group == "forms") group_forms();
  else if (group == "convert") group_convert();
  else if (group == "reorder") group_reorder(tmp);
  else if (group == "generators") group_generators();
  else if (group == "threads") group_threads(tmp);
  else if (group == "refusals") group_refusals();
  else if (group == "loaders") group_loaders(tmp);
  else {
    std::fprintf(stderr, "unknown group %s\n", group.c_str());
    return 2;
  }
  return 0;
}
