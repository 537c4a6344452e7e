// sample_neighbors.hip — neighbour sampling over CSR on the device, gfx950 (contract in
// include/ofx_spmm.h, rules in sample_neighbors.h).
//
//   lengths kernel : out_row_ptr[i + 1] = min(deg(seeds[i]), fanout), the bad flag
//   hipcub scan    : out_row_ptr[1..S] in place -> the sampled row_ptr; its last entry is the total
//   sample kernel  : a group of G lanes serves one seed, G the power of two >= fanout (4..64), so a
//                    wave serves 64 / G seeds.  Lane t computes draw t (philox is counter-based:
//                    the draws of a row do not depend on each other), the group resolves Floyd's
//                    steps in order (step s: lane s's draw is read across the group, the lanes
//                    below s compare it with their final picks, a ballot tells lane s whether to
//                    keep it), each lane ranks its pick by counting the smaller ones, then does its
//                    one gather and its one or two stores.
// O(fanout) work per row whatever its degree: a hub row is a row like any other.  No LDS, no
// atomics, no inter-block traffic; the only cross-lane steps are reads and ballots inside a wave.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include "ofx_internal.h"
#include "sample_neighbors.h"
#include "spmm_common.h"
#include "spmm_plan.h"

namespace ofx {
namespace {

constexpr int kBlock = 256;

template <typename I>
__global__ void __launch_bounds__(kBlock)
    sample_lengths_kernel(const I* __restrict__ row_ptr, const I* __restrict__ seeds, int64_t m,
                          int64_t num_seeds, int fanout, I* __restrict__ out_rp,
                          unsigned int* __restrict__ bad) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int64_t first = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (first == 0) out_rp[0] = (I)0;
  for (int64_t i = first; i < num_seeds; i += stride) {
    const smp::RowOf row = smp::row_of(row_ptr, m, (int64_t)seeds[i], fanout);
    if (row.bad) *bad = 1u;  // every writer stores the same word
    out_rp[i + 1] = (I)row.len;
  }
}

// x of lane s of this lane's group; s is wave-uniform.
template <int G>
__device__ __forceinline__ uint32_t group_read(uint32_t x, int s) {
  if constexpr (G == 64)
    return (uint32_t)__builtin_amdgcn_readlane((int)x, s);
  else
    return (uint32_t)__shfl((int)x, s, G);
}

template <typename I, int G>
__global__ void __launch_bounds__(kBlock)
    sample_kernel(const I* __restrict__ row_ptr, const I* __restrict__ col_idx,
                  const I* __restrict__ seeds, int64_t m, int64_t num_seeds, int fanout,
                  uint64_t seed, const I* __restrict__ rp_s, I* __restrict__ out_col,
                  I* __restrict__ out_eid, int64_t* __restrict__ out_nnz) {
  constexpr uint64_t kGroupMask = G == 64 ? ~0ull : ((1ull << (G & 63)) - 1ull);
  const int64_t thread = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const int64_t i = thread / G;
  const int t = (int)(threadIdx.x & (G - 1));
  const int group_base = (int)(threadIdx.x & 63 & ~(G - 1));
  if (thread == 0) *out_nnz = (int64_t)rp_s[num_seeds];

  // Every lane stays to the end (the cross-lane steps need the whole wave); a lane past the last
  // seed, a bad seed's group and the lanes past a row's length have nothing to store.
  smp::RowOf row{0, 0, 0, true};
  int64_t v = 0;
  if (i < num_seeds) {
    v = (int64_t)seeds[i];
    row = smp::row_of(row_ptr, m, v, fanout);
  }
  const bool live = t < row.len;
  const bool sampled = live && row.deg > (int64_t)fanout;
  // A row of at most `fanout` entries keeps them all: lane t holds position t, already ranked.
  uint32_t pick = live ? (uint32_t)t : 0xffffffffu;  // a dead lane's pick is above every position
  uint32_t rank = (uint32_t)t;
  if (__ballot(sampled) != 0ull) {
    uint32_t j = 0;
    if (sampled) {
      j = (uint32_t)row.deg - (uint32_t)fanout + (uint32_t)t;
      pick = smp::draw((uint64_t)v, (uint32_t)t, seed, j);
    }
    // Floyd's steps in order.  Before step s, lanes below s hold their final picks and lane s its
    // draw.  (In a group that keeps its whole row nothing changes: `sampled` is false.)
    for (int s = 1; s < fanout; ++s) {
      const uint32_t r = group_read<G>(pick, s);
      const uint64_t hits = __ballot(t < s && pick == r);
      const bool taken = ((hits >> group_base) & kGroupMask) != 0ull;
      if (t == s && sampled) pick = smp::floyd_pick(pick, j, taken);
    }
    // The picks of a row are distinct: a pick's place in ascending order is the count of smaller
    // ones.
    rank = 0;
    for (int s = 0; s < fanout; ++s) rank += group_read<G>(pick, s) < pick ? 1u : 0u;
  }
  if (live) {
    const int64_t e = row.begin + (int64_t)pick;
    const int64_t o = (int64_t)rp_s[i] + (int64_t)rank;
    out_col[o] = col_idx[e];
    if (out_eid != nullptr) out_eid[o] = (I)e;
  }
}

int scan_bytes_of(int idx_dtype, int64_t num_seeds, size_t* bytes) {
  *bytes = 0;
  if (num_seeds == 0) return OFX_OK;
  return by_index(idx_dtype, [&](auto* ip) -> int {
    using I = std::remove_pointer_t<decltype(ip)>;
    OFX_HIP_CHECK(hipcub::DeviceScan::InclusiveSum(nullptr, *bytes, (I*)nullptr, (I*)nullptr,
                                                   (int)num_seeds));
    return OFX_OK;
  });
}

struct SampleWs {
  size_t bad, cub, cub_bytes, total;
};

int sample_ws(int idx_dtype, int64_t num_seeds, SampleWs* w) {
  *w = SampleWs{};
  size_t scan = 0;
  const int rc = scan_bytes_of(idx_dtype, num_seeds, &scan);
  if (rc) return rc;
  w->bad = 0;
  w->cub = 256;
  w->cub_bytes = scan;
  w->total = 256 + plan::align_up(scan, 256);
  return OFX_OK;
}

template <typename I, int G>
void launch_sample(hipStream_t s, const I* rp, const I* ci, const I* seeds, int64_t m,
                   int64_t num_seeds, int fanout, uint64_t seed, const I* rp_s, I* out_col,
                   I* out_eid, int64_t* out_nnz) {
  const int64_t blocks = (num_seeds * G + kBlock - 1) / kBlock;
  hipLaunchKernelGGL((sample_kernel<I, G>), dim3((unsigned)blocks), dim3(kBlock), 0, s, rp, ci,
                     seeds, m, num_seeds, fanout, seed, rp_s, out_col, out_eid, out_nnz);
}

template <typename I>
int sample(hipStream_t s, int64_t m, int64_t num_seeds, const I* rp, const I* ci, const I* seeds,
           int fanout, uint64_t seed, I* out_rp, I* out_col, I* out_eid, int64_t* out_nnz,
           unsigned int* bad_out, char* ws, size_t ws_bytes) {
  if (num_seeds == 0) {
    OFX_HIP_CHECK(hipMemsetAsync(out_rp, 0, sizeof(I), s));
    OFX_HIP_CHECK(hipMemsetAsync(out_nnz, 0, sizeof(int64_t), s));
    if (bad_out) OFX_HIP_CHECK(hipMemsetAsync(bad_out, 0, sizeof(unsigned int), s));
    return OFX_OK;
  }
  SampleWs w;
  const int rc = sample_ws(sizeof(I) == 4 ? OFX_DT_INT32 : OFX_DT_INT64, num_seeds, &w);
  if (rc) return rc;
  OFX_REQUIRE(ws && ws_bytes >= w.total, OFX_EWORKSPACE,
              "sample_neighbors: workspace of %zu bytes < %zu required", ws_bytes, w.total);
  auto* bad = bad_out ? bad_out : reinterpret_cast<unsigned int*>(ws + w.bad);
  OFX_HIP_CHECK(hipMemsetAsync(bad, 0, sizeof(unsigned int), s));
  int64_t g = (num_seeds + kBlock - 1) / kBlock;
  if (g > 65536) g = 65536;
  hipLaunchKernelGGL((sample_lengths_kernel<I>), dim3((unsigned)g), dim3(kBlock), 0, s, rp, seeds, m,
                     num_seeds, fanout, out_rp, bad);
  OFX_HIP_CHECK(hipGetLastError());
  size_t cb = w.cub_bytes;
  OFX_HIP_CHECK(hipcub::DeviceScan::InclusiveSum(ws + w.cub, cb, out_rp + 1, out_rp + 1,
                                                 (int)num_seeds, s));
  if (fanout <= 4)
    launch_sample<I, 4>(s, rp, ci, seeds, m, num_seeds, fanout, seed, out_rp, out_col, out_eid, out_nnz);
  else if (fanout <= 8)
    launch_sample<I, 8>(s, rp, ci, seeds, m, num_seeds, fanout, seed, out_rp, out_col, out_eid, out_nnz);
  else if (fanout <= 16)
    launch_sample<I, 16>(s, rp, ci, seeds, m, num_seeds, fanout, seed, out_rp, out_col, out_eid, out_nnz);
  else if (fanout <= 32)
    launch_sample<I, 32>(s, rp, ci, seeds, m, num_seeds, fanout, seed, out_rp, out_col, out_eid, out_nnz);
  else
    launch_sample<I, 64>(s, rp, ci, seeds, m, num_seeds, fanout, seed, out_rp, out_col, out_eid, out_nnz);
  OFX_HIP_CHECK(hipGetLastError());
  return OFX_OK;
}

}  // namespace
}  // namespace ofx

using namespace ofx;

extern "C" int ofx_sample_neighbors_workspace_size(int idx_dtype, int64_t num_seeds, size_t* bytes) {
  return ::ofx::guarded(__func__, [&]() -> int {
    OFX_REQUIRE(bytes && num_seeds >= 0 && num_seeds <= INT32_MAX, OFX_EINVAL,
                "sample_neighbors: bad sizes (num_seeds must be < 2^31)");
    OFX_REQUIRE(is_index_dtype(idx_dtype), OFX_EUNSUPPORTED,
                "sample_neighbors: bad index dtype %d", idx_dtype);
    SampleWs w;
    const int rc = sample_ws(idx_dtype, num_seeds, &w);
    *bytes = w.total;
    return rc;
  });
}

extern "C" int ofx_sample_neighbors(void* stream, int idx_dtype, int64_t m, int64_t num_seeds,
                                    const void* row_ptr, const void* col_idx, const void* seeds,
                                    int fanout, uint64_t seed, void* out_row_ptr, void* out_col_idx,
                                    void* out_edge_ids, void* out_nnz, void* bad_flag,
                                    void* workspace, size_t workspace_bytes) {
  return ::ofx::guarded(__func__, [&]() -> int {
    const int rc = smp::check_sample_args("sample_neighbors", idx_dtype, m, num_seeds, row_ptr,
                                          col_idx, seeds, fanout, out_row_ptr, out_col_idx, out_nnz);
    if (rc) return rc;
    OFX_REQUIRE(num_seeds <= INT32_MAX, OFX_EINVAL, "sample_neighbors: num_seeds must be < 2^31");
    hipStream_t s = static_cast<hipStream_t>(stream);
    return by_index(idx_dtype, [&](auto* ip) -> int {
      using I = std::remove_pointer_t<decltype(ip)>;
      return sample<I>(s, m, num_seeds, (const I*)row_ptr, (const I*)col_idx, (const I*)seeds, fanout,
                       seed, (I*)out_row_ptr, (I*)out_col_idx, (I*)out_edge_ids, (int64_t*)out_nnz,
                       (unsigned int*)bad_flag, (char*)workspace, workspace_bytes);
    });
  });
}
