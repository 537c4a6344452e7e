// csr_host_cpu.cpp — the host utilities of the CSR itself (no dense operand): the row partition
// (BalancedSplitter), the row slice of a row_ptr, values gathered through a permutation, the
// transpose and COO -> CSR.  The latter two are the DeviceType::kCPU kernels of ops
// "csr_transpose" and the COO builder, with the same output as spmm_backward.hip / csr_build.hip.
#pragma clang fp contract(off)

#include <algorithm>
#include <numeric>
#include <vector>

#include "ofx_internal.h"
#include "spmm_common.h"
#include "spmm_rows_cpu.h"

using namespace ofx;

// ---- BalancedSplitter (oneflow/core/common/balanced_splitter.cpp:20-40) -------------------
extern "C" int ofx_balanced_range(int64_t total, int64_t parts, int64_t idx, int64_t* begin,
                                  int64_t* end) {
  return ::ofx::guarded(__func__, [&]() -> int {
    OFX_REQUIRE(total >= 0 && parts > 0 && idx >= 0 && idx < parts && begin && end, OFX_EINVAL,
                "balanced_range: bad arguments (total=%lld parts=%lld idx=%lld)", (long long)total,
                (long long)parts, (long long)idx);
    const int64_t base = total / parts, extra = total % parts;
    // The first `extra` parts hold base+1 elements.
    const int64_t lo = idx < extra ? idx * (base + 1) : extra * (base + 1) + (idx - extra) * base;
    *begin = lo;
    *end = lo + base + (idx < extra ? 1 : 0);
    return OFX_OK;
  });
}

extern "C" int ofx_csr_row_slice_host(int idx_dtype, const void* row_ptr, int64_t row_begin,
                                      int64_t row_end, void* out_row_ptr, int64_t* nnz_begin,
                                      int64_t* nnz_end) {
  return ::ofx::guarded(__func__, [&]() -> int {
    OFX_REQUIRE(is_index_dtype(idx_dtype), OFX_EUNSUPPORTED, "csr_row_slice_host: bad dtype");
    OFX_REQUIRE(row_ptr && 0 <= row_begin && row_begin <= row_end, OFX_EINVAL,
                "csr_row_slice_host: bad arguments");
    return by_index(idx_dtype, [&](auto* ip) -> int {
      using I = std::remove_pointer_t<decltype(ip)>;
      const I* rp = static_cast<const I*>(row_ptr);
      I* out = static_cast<I*>(out_row_ptr);
      const int64_t base = (int64_t)rp[row_begin];
      if (out)
        for (int64_t i = 0; i <= row_end - row_begin; ++i)
          out[i] = (I)((int64_t)rp[row_begin + i] - base);
      if (nnz_begin) *nnz_begin = base;
      if (nnz_end) *nnz_end = (int64_t)rp[row_end];
      return OFX_OK;
    });
  });
}

extern "C" int ofx_gather_values_host(int idx_dtype, int val_dtype, int64_t nnz, const void* perm,
                                      const void* src, void* dst) {
  return ::ofx::guarded(__func__, [&]() -> int {
    OFX_REQUIRE(is_index_dtype(idx_dtype), OFX_EUNSUPPORTED, "gather_values: bad index dtype %d",
                idx_dtype);
    const int vs = dtype_size(val_dtype);
    OFX_REQUIRE(vs == 2 || vs == 4 || vs == 8, OFX_EUNSUPPORTED, "gather_values: bad value dtype %d",
                val_dtype);
    OFX_REQUIRE(nnz >= 0 && (nnz == 0 || (perm && src && dst)), OFX_EINVAL,
                "gather_values: NULL argument");
    const char* s = static_cast<const char*>(src);
    char* d = static_cast<char*>(dst);
    return by_index(idx_dtype, [&](auto* ip) -> int {
      using I = std::remove_pointer_t<decltype(ip)>;
      for (int64_t t = 0; t < nnz; ++t) {
        const int64_t j = (int64_t) static_cast<const I*>(perm)[t];
        OFX_REQUIRE(j >= 0 && j < nnz, OFX_EINVAL,
                    "gather_values: perm[%lld] = %lld outside [0, %lld)", (long long)t,
                    (long long)j, (long long)nnz);
        memcpy(d + (size_t)t * vs, s + (size_t)j * vs, (size_t)vs);
      }
      return OFX_OK;
    });
  });
}

// ---- transpose (same output as csrc/spmm_backward.hip) -----------------------------------------
namespace {

template <typename I>
void cpu_transpose(int64_t m, int64_t k, int64_t nnz, const I* rp, const I* col, I* out_rp,
                   I* out_col, I* out_perm) {
  // key k for a column outside [0, k): after row_ptr_T[k], never read (csrc/spmm_backward.hip
  // transpose_keys_kernel)
  auto key = [&](int64_t j) {
    const int64_t c = (int64_t)col[j];
    return (uint64_t)c < (uint64_t)k ? c : k;
  };
  std::vector<int64_t> cnt(k + 2, 0);
  for (int64_t j = 0; j < nnz; ++j) ++cnt[key(j) + 1];
  for (int64_t c = 0; c <= k; ++c) cnt[c + 1] += cnt[c];
  for (int64_t c = 0; c <= k; ++c) out_rp[c] = (I)cnt[c];
  for (int64_t r = 0; r < m; ++r)  // rows ascending -> stable within each column
    for (int64_t j = (int64_t)rp[r]; j < (int64_t)rp[r + 1]; ++j) {
      const int64_t pos = cnt[key(j)]++;
      out_col[pos] = (I)r;
      out_perm[pos] = (I)j;
    }
}

}  // namespace

extern "C" int ofx_csr_transpose_cpu(int idx_dtype, int64_t m, int64_t k, int64_t nnz,
                                     const void* row_ptr, const void* col_idx, void* out_row_ptr,
                                     void* out_col_idx, void* out_perm) {
  return ::ofx::guarded(__func__, [&]() -> int {
    OFX_REQUIRE(m >= 0 && k >= 0 && nnz >= 0 && row_ptr && out_row_ptr &&
                    (nnz == 0 || (col_idx && out_col_idx && out_perm)),
                OFX_EINVAL, "csr_transpose_cpu: bad arguments");
    OFX_REQUIRE(is_index_dtype(idx_dtype), OFX_EUNSUPPORTED, "csr_transpose_cpu: bad index dtype %d",
                idx_dtype);
    return by_index(idx_dtype, [&](auto* ip) -> int {
      using I = std::remove_pointer_t<decltype(ip)>;
      OFX_REQUIRE(!negative_column((const I*)col_idx, 0, nnz), OFX_EINVAL,
                  "csr_transpose_cpu: negative column index (gather_kernel_util.cpp:80 "
                  "CHECK_GE(idx, 0))");
      cpu_transpose<I>(m, k, nnz, (const I*)row_ptr, (const I*)col_idx, (I*)out_row_ptr,
                       (I*)out_col_idx, (I*)out_perm);
      return OFX_OK;
    });
  });
}

// ---- COO -> CSR on the host (same output as csr_build.hip) ------------------------------------
namespace {

template <typename T, typename I>
int64_t cpu_coo_to_csr(int64_t m, int64_t k, int64_t nnz, const I* row, const I* col, const T* val,
                       int merge, I* out_rp, I* out_col, T* out_val) {
#pragma clang fp contract(off)
  using A = typename Num<T>::acc;
  std::vector<int64_t> perm(nnz);
  std::iota(perm.begin(), perm.end(), 0);
  auto key = [&](int64_t i) { return (uint64_t)row[i] * (uint64_t)k + (uint64_t)col[i]; };
  std::stable_sort(perm.begin(), perm.end(), [&](int64_t a, int64_t b) { return key(a) < key(b); });
  int64_t o = 0;
  std::vector<int64_t> cnt(m + 1, 0);
  for (int64_t i = 0; i < nnz;) {
    int64_t e = i + 1;
    if (merge)
      while (e < nnz && key(perm[e]) == key(perm[i])) ++e;
    out_col[o] = col[perm[i]];
    if (val) {
      A acc = A(0);
      for (int64_t q = i; q < e; ++q) acc = acc + Num<T>::load(val[perm[q]]);
      out_val[o] = Num<T>::store(acc);
    }
    ++cnt[(int64_t)row[perm[i]] + 1];
    ++o;
    i = e;
  }
  for (int64_t r = 0; r < m; ++r) cnt[r + 1] += cnt[r];
  for (int64_t r = 0; r <= m; ++r) out_rp[r] = (I)cnt[r];
  return o;
}

}  // namespace

extern "C" int ofx_coo_to_csr_cpu(int idx_dtype, int val_dtype, int64_t m, int64_t k, int64_t nnz,
                                  const void* row, const void* col, const void* values,
                                  int merge_duplicates, void* out_row_ptr, void* out_col_idx,
                                  void* out_values, int64_t* out_nnz) {
  return ::ofx::guarded(__func__, [&]() -> int {
    OFX_REQUIRE(m >= 0 && k >= 0 && nnz >= 0 && out_row_ptr && out_nnz &&
                    (nnz == 0 || (row && col && out_col_idx)),
                OFX_EINVAL, "coo_to_csr_cpu: bad arguments");
    OFX_REQUIRE(is_index_dtype(idx_dtype), OFX_EUNSUPPORTED, "coo_to_csr_cpu: bad index dtype");
    OFX_REQUIRE((values == nullptr) == (out_values == nullptr), OFX_EINVAL,
                "coo_to_csr_cpu: values and out_values must both be given or both be NULL");
    const int in_range = by_index(idx_dtype, [&](auto* ip) -> int {
      using I = std::remove_pointer_t<decltype(ip)>;
      const I* r = (const I*)row;
      const I* c = (const I*)col;
      for (int64_t i = 0; i < nnz; ++i)
        OFX_REQUIRE(r[i] >= 0 && r[i] < m && c[i] >= 0 && c[i] < k, OFX_EINVAL,
                    "coo_to_csr_cpu: entry %lld (%lld, %lld) outside %lld x %lld", (long long)i,
                    (long long)r[i], (long long)c[i], (long long)m, (long long)k);
      return OFX_OK;
    });
    if (in_range != OFX_OK) return in_range;
    const int vdt = values ? val_dtype : OFX_DT_FLOAT;  // no values: any type, never read
    OFX_REQUIRE(is_value_dtype(vdt), OFX_EUNSUPPORTED, "coo_to_csr_cpu: bad value dtype %d", vdt);
    return by_types(idx_dtype, vdt, [&](auto* tp, auto* ip) -> int {
      using T = std::remove_pointer_t<decltype(tp)>;
      using I = std::remove_pointer_t<decltype(ip)>;
      *out_nnz = cpu_coo_to_csr<T, I>(m, k, nnz, (const I*)row, (const I*)col, (const T*)values,
                                      merge_duplicates, (I*)out_row_ptr, (I*)out_col_idx,
                                      (T*)out_values);
      return OFX_OK;
    });
  });
}
