// random_walk.hip — random walks over CSR on the device, uniform and node2vec, gfx950 (contract in
// include/ofx_spmm.h, rules in random_walk.h).
//
// A walk is a chain of `length` dependent gathers (row_ptr[v], then col_idx[e]), so a kernel's
// rate is the number of walks in flight over the latency of a step, and the cost of its output is
// how the stores of a wave fall onto the rows of `walks`, which lie (length + 1) entries apart.
//
//   walk_first_order_kernel  : p == q == 1, every attempt 0 is accepted.  One lane per walk.  The
//                              block stages T steps of its 256 walks in LDS (T: 64 bytes of a
//                              walk's row; row stride T + 1, so a step's column and a walk's row
//                              both spread over the banks) and flushes the tile with flat
//                              indexing, T consecutive lanes writing one contiguous run of a
//                              walk's row.  Against one strided store per lane and step this
//                              took 0.76 of the time at 40 and 80 steps.
//   walk_second_order_kernel : a group of G lanes per walk.  The generator is counter-based, so
//                              in round k lane g computes attempt k * G + g in full (words,
//                              candidate gather, class against the previous node by binary search
//                              over its row, whose bounds stay in registers); a ballot masked to
//                              the group gives the lowest accepted attempt, whose node and entry
//                              are read across the group: the sequential rule's answer with the
//                              dependent chain cut from rejections to rounds.  Lane t mod G latches
//                              step t, and every G steps the group stores G consecutive entries of
//                              its walk's row; no LDS.
// Every lane stays to the end of its block; no atomics but the same-word store of the bad flag.
// Every read, a losing attempt's included, is inside a row whose bounds were checked when read.
#include <hip/hip_runtime.h>

#include "ofx_internal.h"
#include "random_walk.h"
#include "spmm_common.h"

namespace ofx {
namespace {

constexpr int kBlock = 256;
constexpr int kGroup = 8;  // lanes per second-order walk

// Steps a first-order block stages per walk: 64 bytes of a walk's row.
template <typename I>
constexpr int tile_steps() {
  return 64 / (int)sizeof(I);
}

// Walk i's start and the row it stands on; a start outside [0, m) is flagged and ends the walk.
template <typename I>
__device__ __forceinline__ rw::Row start_of(const I* __restrict__ row_ptr,
                                            const I* __restrict__ starts, int64_t m, int64_t nnz,
                                            int64_t i, int64_t num_walks, int64_t* v,
                                            unsigned int* __restrict__ bad) {
  *v = -1;
  if (i >= num_walks) return rw::Row{0, 0, true, false};
  *v = (int64_t)starts[i];
  if ((*v < 0 || *v >= m) && bad != nullptr) *bad = 1u;  // every writer stores the same word
  return rw::row_of(row_ptr, m, nnz, *v);
}

template <typename I, bool E>
__global__ void __launch_bounds__(kBlock)
    walk_first_order_kernel(const I* __restrict__ row_ptr, const I* __restrict__ col_idx,
                            const I* __restrict__ starts, int64_t m, int64_t nnz, int64_t num_walks,
                            int length, uint64_t seed, I* __restrict__ walks, I* __restrict__ eids,
                            unsigned int* __restrict__ bad) {
  constexpr int T = tile_steps<I>();
  constexpr int kStride = T + 1;
  __shared__ I tile[(E ? 2 : 1) * kBlock * kStride];
  I* const etile = tile + kBlock * kStride;
  const int lane = (int)threadIdx.x;
  const int64_t wbase = (int64_t)blockIdx.x * kBlock;
  const int64_t i = wbase + lane;
  const int64_t row_len = (int64_t)length + 1;

  int64_t v;
  rw::Row row = start_of(row_ptr, starts, m, nnz, i, num_walks, &v, bad);
  int64_t e = -1;
  for (int t = 0; t <= length; ++t) {
    if (t > 0) {
      if (row.bad && bad != nullptr) *bad = 1u;
      e = -1;
      if (!row.ended) {
        uint32_t w0, w1;
        rw::attempt_words((uint64_t)i, (uint32_t)t, 0u, seed, &w0, &w1);
        e = rw::candidate(row.begin, row.end - row.begin, w0);
        v = (int64_t)col_idx[e];
        if (t < length) row = rw::row_of(row_ptr, m, nnz, v);  // the last node's row is not read
      } else {
        v = -1;
      }
    }
    const int col = t % T;
    tile[lane * kStride + col] = (I)v;
    if (E) etile[lane * kStride + col] = (I)e;
    if (col == T - 1 || t == length) {
      // steps t0 .. t of the block's walks: T consecutive lanes write one run of a walk's row
      const int t0 = t - col;
      __syncthreads();
#pragma unroll 2  // unrolled in full, the flush alone would hold 100 registers
      for (int k = 0; k < T; ++k) {
        const int f = k * kBlock + lane;
        const int wl = f / T, st = f % T;
        const int64_t wi = wbase + wl;
        if (st <= col && wi < num_walks) {
          walks[wi * row_len + t0 + st] = tile[wl * kStride + st];
          if (E && t0 + st >= 1) eids[wi * (int64_t)length + t0 + st - 1] = etile[wl * kStride + st];
        }
      }
      __syncthreads();
    }
  }
}

template <typename I, int G>
__global__ void __launch_bounds__(kBlock)
    walk_second_order_kernel(const I* __restrict__ row_ptr, const I* __restrict__ col_idx,
                             const I* __restrict__ starts, int64_t m, int64_t nnz,
                             int64_t num_walks, int length, uint64_t seed, rw::Thresholds th,
                             I* __restrict__ walks, I* __restrict__ eids,
                             unsigned int* __restrict__ bad) {
  static_assert(G >= 2 && G <= 32 && (G & (G - 1)) == 0 && rw::kMaxAttempts % G == 0,
                "a group is a power of two of lanes inside a wave that divides the attempt cap");
  constexpr uint64_t kGroupMask = (1ull << G) - 1ull;
  const int64_t i = ((int64_t)blockIdx.x * kBlock + threadIdx.x) / G;
  const int g = (int)(threadIdx.x & (G - 1));
  const int group_base = (int)(threadIdx.x & 63 & ~(G - 1));
  const int64_t row_len = (int64_t)length + 1;
  const bool search = th.thr[rw::kCommon] != th.thr[rw::kOut];
  const bool stores = i < num_walks;

  int64_t v;
  rw::Row row = start_of(row_ptr, starts, m, nnz, i, num_walks, &v, bad);
  int64_t u = -1, ub = 0, ue = 0;  // the previous node and its row, from the step that read them
  I node_latch = (I)v;             // lane t mod G holds step t's node until the group stores
  I eid_latch = (I)-1;             // lane (t - 1) mod G holds step t's entry
  for (int t = 1; t <= length; ++t) {
    if (row.bad && bad != nullptr) *bad = 1u;
    int e = -1;  // the accepted entry (nnz < 2^31) and its node
    I xi = (I)-1;
    bool pending = !row.ended;
    const int64_t deg = row.end - row.begin;
    // Round k: lane g computes attempt k * G + g.  The loop is wave-uniform; a group that is done
    // or has ended computes nothing.  The round that holds attempt 255 forces its accept bit.
    for (uint32_t a = (uint32_t)g; __ballot(pending) != 0ull; a += (uint32_t)G) {
      bool accept = false;
      int ce = 0;
      I cx = (I)0;
      if (pending) {
        uint32_t w0, w1;
        rw::attempt_words((uint64_t)i, (uint32_t)t, a, seed, &w0, &w1);
        ce = (int)rw::candidate(row.begin, deg, w0);
        cx = col_idx[ce];
        accept = t == 1 || a == (uint32_t)(rw::kMaxAttempts - 1) ||
                 (uint64_t)w1 < rw::threshold(th, rw::class_of(col_idx, u, ub, ue, (int64_t)cx, search));
      }
      const uint64_t votes = (__ballot(accept) >> group_base) & kGroupMask;
      const int win = votes != 0ull ? __ffsll((unsigned long long)votes) - 1 : 0;
      const int we = __shfl(ce, win, G);
      const I wx = __shfl(cx, win, G);
      if (pending && votes != 0ull) {  // group-uniform
        e = we;
        xi = wx;
        pending = false;
      }
    }
    if (!row.ended) {
      u = v;
      ub = row.begin;
      ue = row.end;
      v = (int64_t)xi;
      if (t < length) row = rw::row_of(row_ptr, m, nnz, v);  // the last node's row is not read
    } else {
      v = -1;
    }
    if (t % G == g) node_latch = xi;
    if ((t - 1) % G == g) eid_latch = (I)e;
    if (stores) {
      const int c = t % G;
      if ((c == G - 1 || t == length) && g <= c) walks[i * row_len + (t - c) + g] = node_latch;
      const int d = (t - 1) % G;
      if (eids != nullptr && (d == G - 1 || t == length) && g <= d)
        eids[i * (int64_t)length + (t - 1 - d) + g] = eid_latch;
    }
  }
}

template <typename I>
int walk(hipStream_t s, int64_t m, int64_t nnz, int64_t num_walks, const I* rp, const I* ci,
         const I* starts, int length, const rw::Thresholds& th, uint64_t seed, I* walks, I* eids,
         unsigned int* bad) {
  if (bad) OFX_HIP_CHECK(hipMemsetAsync(bad, 0, sizeof(unsigned int), s));
  if (num_walks == 0) return OFX_OK;
  if (rw::first_order(th)) {
    const dim3 grid((unsigned)((num_walks + kBlock - 1) / kBlock));
    if (eids != nullptr)
      hipLaunchKernelGGL((walk_first_order_kernel<I, true>), grid, dim3(kBlock), 0, s, rp, ci,
                         starts, m, nnz, num_walks, length, seed, walks, eids, bad);
    else
      hipLaunchKernelGGL((walk_first_order_kernel<I, false>), grid, dim3(kBlock), 0, s, rp, ci,
                         starts, m, nnz, num_walks, length, seed, walks, eids, bad);
  } else {
    const dim3 grid((unsigned)((num_walks * kGroup + kBlock - 1) / kBlock));
    hipLaunchKernelGGL((walk_second_order_kernel<I, kGroup>), grid, dim3(kBlock), 0, s, rp, ci,
                       starts, m, nnz, num_walks, length, seed, th, walks, eids, bad);
  }
  OFX_HIP_CHECK(hipGetLastError());
  return OFX_OK;
}

}  // namespace
}  // namespace ofx

using namespace ofx;

extern "C" int ofx_random_walk(void* stream, int idx_dtype, int64_t m, int64_t nnz,
                               int64_t num_walks, const void* row_ptr, const void* col_idx,
                               const void* starts, int length, double p, double q, uint64_t seed,
                               void* out_walks, void* out_edge_ids, void* bad_flag) {
  return ::ofx::guarded(__func__, [&]() -> int {
    rw::Thresholds th;
    const int rc = rw::check_walk_args("random_walk", idx_dtype, m, nnz, num_walks, row_ptr,
                                       col_idx, starts, length, p, q, out_walks, &th);
    if (rc) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    return by_index(idx_dtype, [&](auto* ip) -> int {
      using I = std::remove_pointer_t<decltype(ip)>;
      return walk<I>(s, m, nnz, num_walks, (const I*)row_ptr, (const I*)col_idx, (const I*)starts,
                     length, th, seed, (I*)out_walks, (I*)out_edge_ids, (unsigned int*)bad_flag);
    });
  });
}
