// sddmm_heads.hip — the multi-head SDDMM over a CSR pattern (op "sddmm_csr_heads"), gfx950:
//   out[j, h] = <a[row(j), h*D:(h+1)*D], b[col[j], h*D:(h+1)*D]>
// for H heads of width D (out is [nnz, H] row-major): the scores of multi-head graph attention
// and d(values) of spmm_csr_heads.  Contract (include/ofx_spmm.h): ofx_sddmm_csr's
// order WITHIN the head -- products rounded, leaves of 8 consecutive columns of the head summed
// sequentially from +0, the head's leaves zero-padded to a power of two and added pairwise, one
// rounding to T.  Leaves never straddle heads.
//
// Work items as the narrow SDDMM's (spmm_backward.hip): a lane group per row or hub chunk of the
// shared planner's work list (skip_empty; the cut has no numeric effect), the `a` row in registers
// for the whole item, B rows streamed U nonzeros in flight.
//   Fast path (D % 8 == 0, D / 8 a power of two, H*D <= 2048, 16-byte-aligned rows): the group
//   covers all H*D columns, lane t owning the L leaves [t*L, (t+1)*L); the B row is read once with
//   16-byte loads.  A head is D/8 consecutive leaves: the pairwise tree runs in the lane over the
//   head's leaves it holds, then as an xor butterfly restricted to the head's lanes (a segmented
//   butterfly).  The first lane of each head stores its result: the H results of a nonzero are
//   contiguous.
//   General path (any other (H, D) with D <= 2048, or unaligned rows): a lane group per (item,
//   head) with column base h*D and output stride H, scalar loads; the head's leaves are the
//   group's, so the butterfly is the whole group's and the bits are the same by construction.
// No atomics, no allocation, no host synchronisation.
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>

#include "spmm_extremum.h"
#include "spmm_items_dev.h"

namespace ofx {
namespace {

using namespace item;

constexpr int kLeaf = 8;
constexpr int64_t kHeadsChunk = 256;          // items of at most this many nonzeros (work only)
constexpr int64_t kMaxHeadsN = 256 * kLeaf;   // 64 lanes x 4 leaves

// A lane's leaf in the accumulation type; columns >= n read as +0.
template <typename T, bool ALIGNED>
__device__ __forceinline__ void load_leaf(const T* __restrict__ row, int64_t cb, int64_t n,
                                          typename Num<T>::acc (&x)[kLeaf]) {
  using A = typename Num<T>::acc;
  T raw[kLeaf];
  load_cols<T, kLeaf, ALIGNED>(row, cb, n, Num<T>::store(A(0)), raw);
#pragma unroll
  for (int e = 0; e < kLeaf; ++e) x[e] = Num<T>::load(raw[e]);
}

template <typename T, typename I>
__device__ __forceinline__ bool poison_head_nonzeros(const unsigned long long* __restrict__ counters,
                                                     int64_t block_base, unsigned* err,
                                                     const I* __restrict__ rp, int64_t row_begin,
                                                     int64_t nrows, int64_t heads,
                                                     T* __restrict__ out) {
  if (!plan_failed(counters, block_base, err)) return false;
  const int64_t e0 = (int64_t)rp[row_begin] * heads, e1 = (int64_t)rp[row_begin + nrows] * heads;
  const T p = poison_value<T>();
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t e = e0 + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < e1; e += stride)
    out[e] = p;
  return true;
}

// FAST: the group covers the n = H*D columns of an item, a head is `lh` = D/8 leaves (a power of
// two).  !FAST: group index = item * H + head; the group covers the head's D columns.
template <typename T, typename I, int LG, int L, int U, bool FAST>
__global__ void __launch_bounds__(kBlock)
    sddmm_heads_kernel(const I* __restrict__ rp, const I* __restrict__ col,
                       const T* __restrict__ a, int64_t lda, const T* __restrict__ B, int64_t ldb,
                       int64_t kb, T* __restrict__ out, int64_t row_begin, int64_t nrows,
                       int64_t heads, int64_t d, int lh, int64_t chunk,
                       const unsigned long long* __restrict__ counters,
                       const int64_t* __restrict__ items, const int64_t* __restrict__ order,
                       int64_t block_base, unsigned* err) {
#pragma clang fp contract(off)
  using A = typename Num<T>::acc;
  constexpr int GPW = 64 / LG;
  if (poison_head_nonzeros(counters, block_base, err, rp, row_begin, nrows, heads, out)) return;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int gl = lane & (LG - 1);
  const int gbase = lane & ~(LG - 1);
  const int64_t g = ((block_base + (int64_t)blockIdx.x) * (kBlock / 64) + wave) * GPW + lane / LG;
  const int64_t gi = FAST ? g : g / heads;
  const int64_t head = FAST ? 0 : g - gi * heads;
  Item it;
  if (!work_item<I>(rp, gi, row_begin, nrows, chunk, counters, items, order, &it, true)) return;
  // the columns the group covers: [col0, col0 + w)
  const int64_t col0 = FAST ? 0 : head * d;
  const int64_t w = FAST ? heads * d : d;
  // the tree: `lin` leaves of a head inside a lane, then `seg` lanes of a head
  const int lin = FAST ? (lh < L ? lh : L) : L;
  const int seg = FAST ? (lh / lin) : LG;
  A av[L][kLeaf];
  int hsel[L];  // FAST: the head whose result this lane's leaf l holds after the tree, or -1
#pragma unroll
  for (int l = 0; l < L; ++l) {
    load_leaf<T, FAST>(a + it.lr * lda + col0, (int64_t)(gl * L + l) * kLeaf, w, av[l]);
    hsel[l] = -1;
    if constexpr (FAST) {
      const int gleaf = gl * L + l;
      const int h = gleaf / lh;
      if ((l & (lin - 1)) == 0 && gleaf - h * lh == 0 && h < heads) hsel[l] = h;
    }
  }
  for (int64_t jb = it.j0; jb < it.j1; jb += LG) {
    const int cnt = (int)((it.j1 - jb) < LG ? (it.j1 - jb) : LG);
    const I myc = gl < cnt ? col[jb + gl] : I(0);
    for (int k = 0; k < cnt; k += U) {
      A bv[U][L][kLeaf];
      if constexpr (FAST) {
        // Every load of the round is unconditional and stays a 16-byte word until all are issued
        // (kb > 0 here, sd_heads_typed; as spmm_heads.hip): a slot past the batch's end repeats
        // the batch's last nonzero, a column outside [0, k) reads row 0, a leaf past the row's
        // width reads leaf 0; the last two are then replaced by zeros.
        constexpr int Q = kLeaf * (int)sizeof(T) / 16, PER = 16 / (int)sizeof(T);
        struct Words {
          T v[PER];
        };
        static_assert(sizeof(Words) == sizeof(u32x4), "a 16-byte piece of a leaf");
        u32x4 raw[U][L][Q];
        unsigned inmask = 0;
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const int ku = k + u < cnt ? k + u : cnt - 1;
          const int64_t cu = (int64_t)__shfl((int64_t)myc, gbase + (ku & (LG - 1)), 64);
          const bool in = (uint64_t)cu < (uint64_t)kb;
          inmask |= (in ? 1u : 0u) << u;
          const T* brow = B + (in ? cu : 0) * ldb;
#pragma unroll
          for (int l = 0; l < L; ++l) {
            const int64_t cb = (int64_t)(gl * L + l) * kLeaf;
            const u32x4* src = reinterpret_cast<const u32x4*>(brow + (cb < w ? cb : 0));
#pragma unroll
            for (int q = 0; q < Q; ++q) raw[u][l][q] = src[q];
          }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
#pragma unroll
          for (int l = 0; l < L; ++l) {
            const bool keep = ((inmask >> u) & 1u) != 0 && (int64_t)(gl * L + l) * kLeaf < w;
#pragma unroll
            for (int q = 0; q < Q; ++q) {
              const u32x4 r = keep ? raw[u][l][q] : u32x4{0u, 0u, 0u, 0u};
              const Words wd = __builtin_bit_cast(Words, r);
#pragma unroll
              for (int e = 0; e < PER; ++e) bv[u][l][q * PER + e] = Num<T>::load(wd.v[e]);
            }
          }
        }
      } else {
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const int64_t cu = (int64_t)__shfl((int64_t)myc, gbase + ((k + u) & (LG - 1)), 64);
          if (k + u < cnt) {
            // a column outside [0, k): the forward gathered a zero row; every leaf reads as out
            // of range and the row's address is never used
            const bool in = (uint64_t)cu < (uint64_t)kb;
#pragma unroll
            for (int l = 0; l < L; ++l)
              load_leaf<T, false>(B + (in ? cu : 0) * ldb + col0,
                                  in ? (int64_t)(gl * L + l) * kLeaf : w, w, bv[u][l]);
          }
        }
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (k + u < cnt) {
          const int64_t j = jb + k + u;
          A leaf[L];
#pragma unroll
          for (int l = 0; l < L; ++l) {
            A s = A(0);
#pragma unroll
            for (int e = 0; e < kLeaf; ++e) s = s + av[l][e] * bv[u][l][e];
            leaf[l] = s;
          }
          // pairwise over the head's leaves in this lane (x < lin: pairs never cross a head)
#pragma unroll
          for (int x = 1; x < L; x <<= 1) {
            if (x < lin) {
#pragma unroll
              for (int l = 0; l < L; l += 2 * x) leaf[l] = leaf[l] + leaf[l + x];
            }
          }
          // the butterfly over the head's lanes (seg > 1 only when the lane holds one head)
          A t = leaf[0];
#pragma unroll
          for (int x = 1; x < LG; x <<= 1)
            if (x < seg) t = t + __shfl_xor(t, x, 64);
          leaf[0] = t;
          if constexpr (FAST) {
#pragma unroll
            for (int l = 0; l < L; ++l)
              // a plain store: the H results of a nonzero are a 16-32 byte piece of a line, and
              // the pieces of consecutive nonzeros merge in L2 (non-temporal, the pieces went out
              // one by one: 11-12.7 ms for f32 N = 128 on the products graph)
              if (hsel[l] >= 0) out[j * heads + hsel[l]] = Num<T>::store(leaf[l]);
          } else {
            if (gl == 0) out[j * heads + head] = Num<T>::store(t);
          }
        }
      }
    }
  }
}

struct SdHeadsArgs {
  hipStream_t s;
  const void *rp, *col, *a, *b;
  void* out;
  int64_t lda, ldb, row_begin, nrows, heads, d, nnz, k;
  void* ws;
  size_t ws_bytes;
};

// Work layout only (every out[j, h] is its own dot product): the narrow SDDMM's items.
Schedule sddmm_heads_schedule() {
  Schedule s = resolve_schedule(1, nullptr);
  s.split = s.chunk = kHeadsChunk;
  return s;
}

template <typename T, typename I, int LG, int L, bool FAST>
int sd_heads_cfg(const SdHeadsArgs& x, int lh) {
  constexpr int U = L >= 4 ? 2 : 4;
  Planned p;
  if (const int rc = prepare_plan<I>("sddmm_csr_heads", x.s, static_cast<const I*>(x.rp),
                                     x.row_begin, x.nrows, x.nnz, x.nnz, 0, 0,
                                     sddmm_heads_schedule(), false, x.ws, x.ws_bytes, &p))
    return rc;
  const int64_t groups = FAST ? p.work : p.work * x.heads;
  return launch_cut_grid(groups, (kBlock / 64) * (64 / LG), [&](dim3 grid, int64_t b0) {
    hipLaunchKernelGGL((sddmm_heads_kernel<T, I, LG, L, U, FAST>), grid, dim3(kBlock), 0, x.s,
                       static_cast<const I*>(x.rp), static_cast<const I*>(x.col),
                       static_cast<const T*>(x.a), x.lda, static_cast<const T*>(x.b), x.ldb, x.k,
                       static_cast<T*>(x.out), x.row_begin, x.nrows, x.heads, x.d, lh, p.chunk,
                       p.wl.counters, p.wl.items, p.wl.order, b0, p.err);
  });
}

template <typename T, typename I>
int sd_heads_typed(const SdHeadsArgs& x) {
  const int64_t n = x.heads * x.d;
  const int64_t lh = x.d / kLeaf;
  // k == 0 (every column out of range) takes the general path: the fast one needs a row 0
  const bool fast = x.d % kLeaf == 0 && (lh & (lh - 1)) == 0 && n <= kMaxHeadsN && x.k > 0 &&
                    rows_aligned(x.a, x.lda, sizeof(T), kLeaf) &&
                    rows_aligned(x.b, x.ldb, sizeof(T), kLeaf);
  if (fast) {
    const int64_t leaves = n / kLeaf;
    if (leaves <= 1) return sd_heads_cfg<T, I, 1, 1, true>(x, (int)lh);
    if (leaves <= 2) return sd_heads_cfg<T, I, 2, 1, true>(x, (int)lh);
    if (leaves <= 4) return sd_heads_cfg<T, I, 4, 1, true>(x, (int)lh);
    if (leaves <= 8) return sd_heads_cfg<T, I, 8, 1, true>(x, (int)lh);
    if (leaves <= 16) return sd_heads_cfg<T, I, 16, 1, true>(x, (int)lh);
    if (leaves <= 32) return sd_heads_cfg<T, I, 32, 1, true>(x, (int)lh);
    if (leaves <= 64) return sd_heads_cfg<T, I, 64, 1, true>(x, (int)lh);
    if (leaves <= 128) return sd_heads_cfg<T, I, 64, 2, true>(x, (int)lh);
    return sd_heads_cfg<T, I, 64, 4, true>(x, (int)lh);
  }
  const int64_t leaves = (x.d + kLeaf - 1) / kLeaf;
  if (leaves <= 1) return sd_heads_cfg<T, I, 1, 1, false>(x, 0);
  if (leaves <= 4) return sd_heads_cfg<T, I, 4, 1, false>(x, 0);
  if (leaves <= 16) return sd_heads_cfg<T, I, 16, 1, false>(x, 0);
  if (leaves <= 64) return sd_heads_cfg<T, I, 64, 1, false>(x, 0);
  return sd_heads_cfg<T, I, 64, 4, false>(x, 0);
}

int check_sd_heads_args(const char* fn, int idx_dtype, int val_dtype, int64_t m, int64_t k,
                        int64_t heads, int64_t d, int64_t nnz) {
  OFX_REQUIRE(heads >= 0 && d >= 0 && (d == 0 || heads <= INT64_MAX / d), OFX_EINVAL,
              "%s: bad heads=%lld / d=%lld", fn, (long long)heads, (long long)d);
  return check_types_sizes(fn, idx_dtype, val_dtype, m, k, heads * d, nnz);
}

}  // namespace
}  // namespace ofx

using namespace ofx;

extern "C" int ofx_sddmm_csr_heads_workspace_size(int idx_dtype, int val_dtype, int64_t m,
                                                  int64_t heads, int64_t d, int64_t nnz,
                                                  size_t* bytes) {
  return ::ofx::guarded(__func__, [&]() -> int {
    OFX_REQUIRE(bytes != nullptr, OFX_EINVAL, "sddmm_csr_heads_workspace_size: bytes is NULL");
    if (const int rc = check_sd_heads_args("sddmm_csr_heads_workspace_size", idx_dtype, val_dtype,
                                           m, 0, heads, d, nnz))
      return rc;
    *bytes = plan::ws_layout(m, nnz, 0, 0, sddmm_heads_schedule()).total;
    return OFX_OK;
  });
}

extern "C" int ofx_sddmm_csr_heads(void* stream, int idx_dtype, int val_dtype, int64_t m, int64_t k,
                                   int64_t heads, int64_t d, int64_t nnz, const void* row_ptr,
                                   const void* col_idx, const void* a, int64_t lda, const void* b,
                                   int64_t ldb, void* out, int64_t row_begin, int64_t row_end,
                                   void* workspace, size_t workspace_bytes) {
  return ::ofx::guarded(__func__, [&]() -> int {
    OFX_TAKE_DEVICE_ERROR("sddmm_csr_heads");  // an earlier launch's loud failure (spmm_plan.h)
    int rc = check_sd_heads_args("sddmm_csr_heads", idx_dtype, val_dtype, m, k, heads, d, nnz);
    if (rc) return rc;
    if ((rc = check_row_range("sddmm_csr_heads", row_begin, row_end, m))) return rc;
    const int64_t n = heads * d;
    OFX_REQUIRE(lda >= n && ldb >= n, OFX_EINVAL, "sddmm_csr_heads: lda=%lld / ldb=%lld < n=%lld",
                (long long)lda, (long long)ldb, (long long)n);
    if (row_end == row_begin || nnz == 0 || heads == 0) return OFX_OK;
    OFX_REQUIRE(d > 0, OFX_EINVAL, "sddmm_csr_heads: d == 0 (use a zero fill)");
    OFX_REQUIRE(d <= kMaxHeadsN, OFX_EUNSUPPORTED,
                "sddmm_csr_heads: d=%lld > %lld is not supported", (long long)d,
                (long long)kMaxHeadsN);
    OFX_REQUIRE(row_ptr && col_idx && out && a && b, OFX_EINVAL, "sddmm_csr_heads: NULL pointer");
    const size_t need =
        plan::ws_layout(row_end - row_begin, nnz, 0, 0, sddmm_heads_schedule()).total;
    OFX_REQUIRE(need == 0 || (workspace != nullptr && workspace_bytes >= need), OFX_EWORKSPACE,
                "sddmm_csr_heads: workspace of %zu bytes is smaller than the %zu bytes required",
                workspace_bytes, need);
    const SdHeadsArgs x{static_cast<hipStream_t>(stream), row_ptr, col_idx, a, b, out, lda, ldb,
                        row_begin, row_end - row_begin, heads, d, nnz, k, workspace,
                        workspace_bytes};
    return by_types(idx_dtype, val_dtype, [&](auto* tp, auto* ip) -> int {
      return sd_heads_typed<std::remove_pointer_t<decltype(tp)>,
                            std::remove_pointer_t<decltype(ip)>>(x);
    });
  });
}
