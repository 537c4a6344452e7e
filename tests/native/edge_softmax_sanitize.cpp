// edge_softmax_sanitize.cpp — the kCPU kernels of the edge softmax (csrc/edge_softmax_cpu.cpp with
// csrc/errors.cpp) compiled from source with -fsanitize=address,undefined and driven over their
// edge cases: empty rows, rows around the 8-element leaf and the power-of-two padding of the tree,
// long rows, row ranges, every value type and both index types, NaN / inf scores, exactly sized
// buffers (a read or write past a row's end is a heap overflow here).  The results are also
// checked against a naive double-precision softmax, so a sanitizer-clean run is a correctness run.
// Built and run by tests/test_edge_softmax_cpu.py::test_cpu_kernels_under_sanitizers.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "sanitize_common.h"

namespace {

template <typename T, typename I>
void run_case(const std::vector<int64_t>& lens, int64_t row_begin, int64_t row_end) {
  using N = ofx::Num<T>;
  const int64_t m = (int64_t)lens.size();
  std::vector<I> rp(m + 1, 0);
  for (int64_t r = 0; r < m; ++r) rp[r + 1] = (I)(rp[r] + lens[r]);
  const int64_t nnz = (int64_t)rp[m];
  // exactly sized heap buffers: ASan flags the first byte outside
  std::vector<T> e(nnz), g(nnz), y(nnz), de(nnz);
  for (int64_t j = 0; j < nnz; ++j) {
    e[j] = N::store((typename N::acc)(8.0 * uniform() - 4.0));
    g[j] = N::store((typename N::acc)(2.0 * uniform() - 1.0));
    y[j] = N::store((typename N::acc)(-5));
    de[j] = N::store((typename N::acc)(-5));
  }
  int rc = ofx_edge_softmax_csr_cpu(3, idx_code<I>(), Code<T>::dt, m, nnz, rp.data(), e.data(),
                                    y.data(), row_begin, row_end, nullptr);
  EXPECT(rc == OFX_OK, "forward rc=%d: %s", rc, ofx_last_error());
  rc = ofx_edge_softmax_csr_grad_cpu(3, idx_code<I>(), Code<T>::dt, m, nnz, rp.data(), y.data(),
                                     g.data(), de.data(), row_begin, row_end, nullptr);
  EXPECT(rc == OFX_OK, "backward rc=%d: %s", rc, ofx_last_error());
  for (int64_t r = 0; r < m; ++r) {
    const bool in = r >= row_begin && r < row_end;
    const int64_t j0 = (int64_t)rp[r], j1 = (int64_t)rp[r + 1];
    if (!in) {
      for (int64_t j = j0; j < j1; ++j)
        EXPECT((double)N::load(y[j]) == -5 && (double)N::load(de[j]) == -5,
               "row %lld outside the range was written", (long long)r);
      continue;
    }
    double mx = -INFINITY, s = 0, d = 0;
    for (int64_t j = j0; j < j1; ++j) mx = std::fmax(mx, (double)N::load(e[j]));
    for (int64_t j = j0; j < j1; ++j) s += std::exp((double)N::load(e[j]) - mx);
    for (int64_t j = j0; j < j1; ++j) {
      const double want = std::exp((double)N::load(e[j]) - mx) / s;
      EXPECT(std::fabs((double)N::load(y[j]) - want) <= Code<T>::tol, "row %lld y[%lld] = %g, want %g",
             (long long)r, (long long)j, (double)N::load(y[j]), want);
      d += (double)N::load(y[j]) * (double)N::load(g[j]);
    }
    for (int64_t j = j0; j < j1; ++j) {
      const double want = (double)N::load(y[j]) * ((double)N::load(g[j]) - d);
      EXPECT(std::fabs((double)N::load(de[j]) - want) <= 4 * Code<T>::tol,
             "row %lld de[%lld] = %g, want %g", (long long)r, (long long)j,
             (double)N::load(de[j]), want);
    }
  }
}

template <typename T, typename I>
void run_type() {
  const std::vector<int64_t> lens = {0, 1, 7, 8, 9, 0, 15, 16, 17, 63, 64, 65, 129, 1025, 3, 0};
  const int64_t m = (int64_t)lens.size();
  run_case<T, I>(lens, 0, m);
  run_case<T, I>(lens, 0, 0);
  run_case<T, I>(lens, 3, 13);
  run_case<T, I>(lens, m - 1, m);
  run_case<T, I>({}, 0, 0);
  run_case<T, I>({0, 0, 0}, 0, 3);
}

void special_values() {
  const int32_t rp[] = {0, 3, 6, 8, 11, 12};
  const float inf = INFINITY, nan = NAN;
  const float e[] = {1, nan, 2, 0.5f, inf, 1, -inf, -inf, 1, -inf, 2, -7.25f};
  float y[12];
  int rc = ofx_edge_softmax_csr_cpu(1, OFX_DT_INT32, OFX_DT_FLOAT, 5, 12, rp, e, y, 0, 5, nullptr);
  EXPECT(rc == OFX_OK, "special rc=%d", rc);
  for (int j = 0; j < 8; ++j) {
    uint32_t bits;
    memcpy(&bits, &y[j], 4);
    EXPECT(bits == 0x7fc00000u, "y[%d] = %08x, want the canonical NaN", j, bits);
  }
  EXPECT(y[9] == 0.0f && !std::signbit(y[9]), "-inf in a finite row gives %g", y[9]);
  EXPECT(y[11] == 1.0f, "a single element gives %g", y[11]);
}

void error_paths() {
  const int32_t rp[] = {0, 1};
  float e[1] = {0}, y[1];
  EXPECT(ofx_edge_softmax_csr_cpu(1, OFX_DT_INT32, OFX_DT_FLOAT, 1, 1, rp, e, y, 0, 2, nullptr) ==
             OFX_EINVAL, "row range past m");
  EXPECT(ofx_edge_softmax_csr_cpu(1, OFX_DT_INT32, OFX_DT_INT32, 1, 1, rp, e, y, 0, 1, nullptr) ==
             OFX_EUNSUPPORTED, "value dtype");
  EXPECT(ofx_edge_softmax_csr_cpu(1, OFX_DT_INT32, OFX_DT_FLOAT, 1, 1, rp, nullptr, y, 0, 1,
                                  nullptr) == OFX_EINVAL, "NULL e");
  EXPECT(ofx_edge_softmax_csr_grad_cpu(1, OFX_DT_INT32, OFX_DT_FLOAT, 1, 1, rp, y, nullptr, e, 0,
                                       1, nullptr) == OFX_EINVAL, "NULL g");
  ofx_spmm_options o = OFX_SPMM_OPTIONS_INIT;
  o.ordered = 1;
  EXPECT(ofx_edge_softmax_csr_cpu(1, OFX_DT_INT32, OFX_DT_FLOAT, 1, 1, rp, e, y, 0, 1, &o) ==
             OFX_OK && y[0] == 1.0f, "options are accepted");
}

}  // namespace

int main() {
  g_rng = 12345;
  run_type<float, int32_t>();
  run_type<float, int64_t>();
  run_type<double, int32_t>();
  run_type<double, int64_t>();
  run_type<ofx::bf16, int32_t>();
  run_type<ofx::bf16, int64_t>();
  run_type<ofx::f16, int32_t>();
  run_type<ofx::f16, int64_t>();
  special_values();
  error_paths();
  if (g_failures) {
    printf("%d failures\n", g_failures);
    return 1;
  }
  printf("OK\n");
  return 0;
}
