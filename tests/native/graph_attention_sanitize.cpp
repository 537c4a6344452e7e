// graph_attention_sanitize.cpp — the kCPU entry of the fused multi-head graph attention
// (csrc/graph_attention_heads_cpu.cpp with the kCPU kernels it runs, csrc/spmm_heads_cpu.cpp and
// csrc/edge_softmax_cpu.cpp, and csrc/errors.cpp) compiled from source with
// -fsanitize=address,undefined and driven over the shared problem of tests/heads_cases.py: row
// lengths cycling over 0..130, every value type and both index types, head shapes including D = 5
// and D = 1, hub chunking (split = chunk = 8), row ranges, exactly sized buffers (a read or write
// past an operand's end is a heap overflow here).  attn and out must have the BYTES of the three
// kCPU entries run one after the other on buffers of their own, and lie within the storage type's
// rounding of a naive attention in double: a sanitizer-clean run is a correctness run.
// Built and run by tests/test_graph_attention_cpu.py::test_cpu_kernel_under_sanitizers.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "sanitize_common.h"

namespace {

template <typename T>
constexpr double tolerance() {  // of out against the naive double attention: |values| <= 1
  return sizeof(T) == 8 ? 1e-12 : (sizeof(T) == 4 ? 1e-5 : 3e-2);
}

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
  std::vector<T> q((size_t)(kRows * n)), k((size_t)(kCols * n)), v((size_t)(kCols * n));
  for (auto* t : {&q, &k, &v})
    for (auto& x : *t) x = make<T>(((double)(int)(next() % 9) - 4) / 4);  // multiples of 1/4

  // the naive attention in double
  std::vector<double> ref((size_t)(kRows * n), 0.0);
  for (int64_t r = 0; r < kRows; ++r)
    for (int64_t h = 0; h < heads; ++h) {
      const int64_t j0 = (int64_t)rp[r], j1 = (int64_t)rp[r + 1];
      std::vector<double> s((size_t)(j1 - j0), 0.0);
      double mx = -1e300, sum = 0;
      for (int64_t j = j0; j < j1; ++j) {
        for (int64_t c = 0; c < d; ++c)
          s[(size_t)(j - j0)] += get(q[(size_t)(r * n + h * d + c)]) *
                                 get(k[(size_t)((int64_t)col[j] * n + h * d + c)]);
        mx = s[(size_t)(j - j0)] > mx ? s[(size_t)(j - j0)] : mx;
      }
      for (auto& x : s) sum += (x = std::exp(x - mx));
      for (int64_t j = j0; j < j1; ++j)
        for (int64_t c = 0; c < d; ++c)
          ref[(size_t)(r * n + h * d + c)] +=
              s[(size_t)(j - j0)] / sum * get(v[(size_t)((int64_t)col[j] * n + h * d + c)]);
    }

  const int it = idx_code<I>(), vt = Code<T>::dt;
  ofx_spmm_options hub = OFX_SPMM_OPTIONS_INIT;
  hub.split_threshold = 8;
  hub.chunk = 8;
  const int64_t ranges[][2] = {{0, kRows}, {0, 0}, {kRows, kRows}, {0, 13}, {3, 17}, {17, kRows}};
  for (const ofx_spmm_options* o : {(const ofx_spmm_options*)nullptr, (const ofx_spmm_options*)&hub}) {
    for (const auto& rg : ranges) {
      const int64_t lo = rg[0], hi = rg[1];
      const T mark = make<T>(-77.0);
      std::vector<T> out((size_t)((hi - lo) * n), mark);  // exactly the range's rows
      std::vector<T> attn((size_t)(nnz * heads), mark);
      std::vector<T> qrows(q.begin() + (size_t)(lo * n), q.begin() + (size_t)(hi * n));
      int rc = ofx_graph_attention_csr_heads_cpu(2, it, vt, kRows, kCols, heads, d, nnz, rp.data(),
                                                 col.data(), qrows.data(), n, k.data(), n, v.data(),
                                                 n, out.data(), n, attn.data(), lo, hi, o);
      EXPECT(rc == OFX_OK, "graph_attention_csr_heads_cpu rc=%d: %s", rc, ofx_last_error());
      // the composition on buffers of its own
      std::vector<T> e((size_t)(nnz * heads), mark), y((size_t)(nnz * heads), mark);
      std::vector<T> want((size_t)((hi - lo) * n), mark);
      rc = ofx_sddmm_csr_heads_cpu(2, it, vt, kRows, kCols, heads, d, nnz, rp.data(), col.data(),
                                   qrows.data(), n, k.data(), n, e.data(), lo, hi);
      EXPECT(rc == OFX_OK, "sddmm_csr_heads_cpu rc=%d: %s", rc, ofx_last_error());
      rc = ofx_edge_softmax_csr_heads_cpu(2, it, vt, kRows, heads, nnz, rp.data(), e.data(),
                                          y.data(), lo, hi, o);
      EXPECT(rc == OFX_OK, "edge_softmax_csr_heads_cpu rc=%d: %s", rc, ofx_last_error());
      rc = ofx_spmm_csr_heads_cpu(2, it, vt, kRows, kCols, heads, d, nnz, rp.data(), col.data(),
                                  y.data(), v.data(), n, want.data(), n, lo, hi, o);
      EXPECT(rc == OFX_OK, "spmm_csr_heads_cpu rc=%d: %s", rc, ofx_last_error());
      EXPECT(attn.size() == y.size() &&
                 (attn.empty() || memcmp(attn.data(), y.data(), attn.size() * sizeof(T)) == 0),
             "H=%lld D=%lld rows [%lld, %lld): attn differs from the composition's",
             (long long)heads, (long long)d, (long long)lo, (long long)hi);
      EXPECT(out.empty() || memcmp(out.data(), want.data(), out.size() * sizeof(T)) == 0,
             "H=%lld D=%lld rows [%lld, %lld): out differs from the composition's",
             (long long)heads, (long long)d, (long long)lo, (long long)hi);
      for (int64_t i = 0; i < (hi - lo) * n; ++i)
        EXPECT(std::fabs(get(out[(size_t)i]) - ref[(size_t)(lo * n + i)]) <= tolerance<T>(),
               "H=%lld D=%lld rows [%lld, %lld) element %lld: %g != %g", (long long)heads,
               (long long)d, (long long)lo, (long long)hi, (long long)i, get(out[(size_t)i]),
               ref[(size_t)(lo * n + i)]);
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
  g_rng = 2026;
  run_types<float>();
  run_types<double>();
  run_types<ofx::bf16>();
  run_types<ofx::f16>();
  // refused arguments return a code, never touch memory
  ofx_spmm_options planned = OFX_SPMM_OPTIONS_INIT;
  planned.planned = 1;
  int32_t rp[2] = {0, 1}, ci[1] = {0};
  float x[4] = {0, 0, 0, 0}, y[4] = {0, 0, 0, 0}, z[4] = {0, 0, 0, 0}, o[4], at[2];
  EXPECT(ofx_graph_attention_csr_heads_cpu(1, OFX_DT_INT32, OFX_DT_FLOAT, 1, 1, 2, 2, 1, rp, ci, x,
                                           4, y, 4, z, 4, o, 4, at, 0, 1, &planned) == OFX_EINVAL,
         "planned accepted");
  EXPECT(ofx_graph_attention_csr_heads_cpu(1, OFX_DT_INT32, OFX_DT_FLOAT, 1, 1, 2, 2, 1, rp, ci, x,
                                           4, y, 4, z, 4, o, 4, nullptr, 0, 1, nullptr) ==
             OFX_EINVAL, "NULL attn accepted");
  EXPECT(ofx_graph_attention_csr_heads_cpu(1, OFX_DT_INT32, OFX_DT_FLOAT, 1, 1, 2, 2, 1, rp, ci, x,
                                           4, y, 4, z, 4, o, 4, y, 0, 1, nullptr) == OFX_EINVAL,
         "attn aliasing k accepted");
  EXPECT(ofx_graph_attention_csr_heads_cpu(1, OFX_DT_INT32, OFX_DT_FLOAT, 1, 1, 1, 4096, 1, rp, ci,
                                           x, 4096, y, 4096, z, 4096, o, 4096, at, 0, 1,
                                           nullptr) == OFX_EUNSUPPORTED, "d > 2048 accepted");
  EXPECT(ofx_graph_attention_csr_heads_cpu(1, OFX_DT_INT32, OFX_DT_FLOAT, 1, 1, 2, 2, 1, rp, ci, x,
                                           4, y, 4, z, 4, o, 4, at, 0, 1, nullptr) == OFX_OK,
         "a valid call refused: %s", ofx_last_error());
  if (g_failures) {
    fprintf(stderr, "%d failures\n", g_failures);
    return 1;
  }
  printf("OK\n");
  return 0;
}
