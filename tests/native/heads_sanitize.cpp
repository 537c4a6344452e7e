// heads_sanitize.cpp — the kCPU kernels of the multi-head SpMM / SDDMM (csrc/spmm_heads_cpu.cpp
// with csrc/errors.cpp) compiled from source with -fsanitize=address,undefined and driven over the
// shared problem of tests/heads_cases.py: row lengths cycling over 0..130, every value type and
// both index types, head shapes including D = 5 and D = 1, hub chunking (split = chunk = 8), row
// ranges, exactly sized buffers (a read or write past an operand's end is a heap overflow here).
// The data are small integers, so every sum is exact and the results must EQUAL a naive double
// loop: a sanitizer-clean run is a correctness run.
// Built and run by tests/test_heads_cpu.py::test_cpu_kernels_under_sanitizers.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "sanitize_common.h"

namespace {

template <typename T>
T make(double x) {
  return ofx::Num<T>::store((typename ofx::Num<T>::acc)x);
}
template <typename T>
double get(T x) {
  return (double)ofx::Num<T>::load(x);
}

const int kLengths[] = {0, 1, 2, 7, 8, 9, 63, 64, 65, 130};
constexpr int64_t kRows = 40, kCols = 256;

template <typename T, typename I>
void run(int64_t heads, int64_t d) {
  const int64_t n = heads * d;
  std::vector<I> rp(kRows + 1, 0), col;
  for (int64_t r = 0; r < kRows; ++r) {
    const int len = kLengths[r % 10];
    const int64_t start = (int64_t)(next() % (uint64_t)(kCols - len + 1));
    for (int j = 0; j < len; ++j) col.push_back((I)(start + j));  // unique, ascending
    rp[r + 1] = (I)col.size();
  }
  const int64_t nnz = (int64_t)col.size();
  std::vector<T> vals((size_t)(nnz * heads)), b((size_t)(kCols * n)), a((size_t)(kRows * n));
  const double tv[4] = {-2, -1, 1, 2};
  for (auto& x : vals) x = make<T>(tv[next() & 3]);
  for (auto& x : b) x = make<T>((double)(int)(next() % 9) - 4);
  for (auto& x : a) x = make<T>((double)(int)(next() % 9) - 4);

  // the naive references: exact in double, and exactly representable
  std::vector<double> ref((size_t)(kRows * n), 0.0), ref_sd((size_t)(nnz * heads), 0.0);
  for (int64_t r = 0; r < kRows; ++r)
    for (int64_t j = (int64_t)rp[r]; j < (int64_t)rp[r + 1]; ++j)
      for (int64_t h = 0; h < heads; ++h)
        for (int64_t c = 0; c < d; ++c) {
          const double bv = get(b[(size_t)((int64_t)col[j] * n + h * d + c)]);
          ref[(size_t)(r * n + h * d + c)] += get(vals[(size_t)(j * heads + h)]) * bv;
          ref_sd[(size_t)(j * heads + h)] += get(a[(size_t)(r * n + h * d + c)]) * bv;
        }

  const int it = idx_code<I>(), vt = Code<T>::dt;
  ofx_spmm_options hub = OFX_SPMM_OPTIONS_INIT;
  hub.split_threshold = 8;
  hub.chunk = 8;
  const int64_t ranges[][2] = {{0, kRows}, {0, 0}, {kRows, kRows}, {0, 13}, {3, 17}, {17, kRows}};
  for (const ofx_spmm_options* o : {(const ofx_spmm_options*)nullptr, (const ofx_spmm_options*)&hub}) {
    for (const auto& rg : ranges) {
      const int64_t lo = rg[0], hi = rg[1];
      std::vector<T> out((size_t)((hi - lo) * n));  // exactly the range's rows
      int rc = ofx_spmm_csr_heads_cpu(2, it, vt, kRows, kCols, heads, d, nnz, rp.data(), col.data(),
                                      vals.data(), b.data(), n, out.data(), n, lo, hi, o);
      EXPECT(rc == OFX_OK, "spmm_csr_heads_cpu rc=%d: %s", rc, ofx_last_error());
      for (int64_t i = 0; i < (hi - lo) * n; ++i)
        EXPECT(get(out[(size_t)i]) == get(make<T>(ref[(size_t)(lo * n + i)])),
               "spmm heads H=%lld D=%lld rows [%lld, %lld) element %lld: %g != %g",
               (long long)heads, (long long)d, (long long)lo, (long long)hi, (long long)i,
               get(out[(size_t)i]), ref[(size_t)(lo * n + i)]);
    }
  }
  for (const auto& rg : ranges) {
    const int64_t lo = rg[0], hi = rg[1];
    const T mark = make<T>(-77.0);
    std::vector<T> out((size_t)(nnz * heads), mark);
    std::vector<T> arows(a.begin() + (size_t)(lo * n), a.begin() + (size_t)(hi * n));
    int rc = ofx_sddmm_csr_heads_cpu(2, it, vt, kRows, kCols, heads, d, nnz, rp.data(), col.data(),
                                     arows.data(), n, b.data(), n, out.data(), lo, hi);
    EXPECT(rc == OFX_OK, "sddmm_csr_heads_cpu rc=%d: %s", rc, ofx_last_error());
    const int64_t e0 = (int64_t)rp[lo] * heads, e1 = (int64_t)rp[hi] * heads;
    for (int64_t e = 0; e < nnz * heads; ++e) {
      const double want = (e >= e0 && e < e1) ? get(make<T>(ref_sd[(size_t)e])) : -77.0;
      EXPECT(get(out[(size_t)e]) == want,
             "sddmm heads H=%lld D=%lld rows [%lld, %lld) element %lld: %g != %g", (long long)heads,
             (long long)d, (long long)lo, (long long)hi, (long long)e, get(out[(size_t)e]), want);
    }
  }
}

template <typename T>
void run_types() {
  const int64_t hd[][2] = {{1, 16}, {2, 4}, {3, 5}, {5, 1}, {4, 16}};
  for (const auto& s : hd) {
    run<T, int32_t>(s[0], s[1]);
    run<T, int64_t>(s[0], s[1]);
  }
}

}  // namespace

int main() {
  g_rng = 2024;
  run_types<float>();
  run_types<double>();
  run_types<ofx::bf16>();
  run_types<ofx::f16>();
  // refused arguments return a code, never touch memory
  ofx_spmm_options planned = OFX_SPMM_OPTIONS_INIT;
  planned.planned = 1;
  int32_t rp[2] = {0, 0};
  float x[4] = {0, 0, 0, 0};
  EXPECT(ofx_spmm_csr_heads_cpu(1, OFX_DT_INT32, OFX_DT_FLOAT, 1, 1, 2, 2, 0, rp, nullptr, nullptr,
                                nullptr, 4, x, 4, 0, 1, &planned) == OFX_EINVAL, "planned accepted");
  EXPECT(ofx_sddmm_csr_heads_cpu(1, OFX_DT_INT32, OFX_DT_FLOAT, 1, 1, 1, 4096, 1, rp, rp, x, 4096,
                                 x, 4096, x, 0, 1) == OFX_EUNSUPPORTED, "d > 2048 accepted");
  if (g_failures) {
    fprintf(stderr, "%d failures\n", g_failures);
    return 1;
  }
  printf("OK\n");
  return 0;
}
