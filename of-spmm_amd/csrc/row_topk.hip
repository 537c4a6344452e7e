// row_topk.hip — per-row top-k selection over CSR on the device, gfx950 (contract in
// include/ofx_spmm.h, rules in row_topk.h).  A radix select, not a sort: keys are
// read into registers (rows up to 512 entries) or streamed from global memory (hub rows) and are
// never written back.
//
//   lengths kernel : out_row_ptr[i + 1] = min(deg_i, k), the bad flag, and two row lists appended
//                    with one atomic per wave and class: rows of 65..512 entries and hub rows
//                    (> 512).  A row's place in a list does not matter: its output slot is fixed
//                    by the scan.
//   hipcub scan    : out_row_ptr[1..M] in place; its last entry is nnz_s.
//   group kernel   : a group of G lanes holds one row, up to 8 keys per lane, position
//                    p = slot * G + lane.  Launched twice: G = 8 over all rows (it serves the rows
//                    of at most 64 entries, eight of them per wave) and G = 64 over the list of
//                    65..512.  Select: the key bits from the top; per bit each lane counts its
//                    candidates with the bit set, a butterfly over the group sums them, and the
//                    group either narrows the candidates to them or selects them and lowers the
//                    count still wanted.  A group whose candidates are all wanted is done, and the
//                    wave leaves the bit loop when every group is.  What is left after the last
//                    bit are equal keys: the first `wanted` of them by position are kept.  Emit:
//                    slot by slot, a ballot of the keep bits and a population count of the group's
//                    lanes below give ascending positions.  No LDS, no atomics.
//   hub kernel     : a block of 256 threads per listed row.  Select: 8-bit digits from the top, a
//                    256-bin histogram in LDS per pass over the keys that match the prefix so
//                    far, a block-wide suffix scan of the bins picks the digit and the count still
//                    wanted; it stops early when the digit's whole bin is wanted.  Emit: the row
//                    once more in chunks of 1024 keys; wave ballots and a table of per-wave counts
//                    in LDS order the chunk, two running bases ("above the threshold", "equal to
//                    it") carry across chunks; one barrier per chunk.
// A row with deg <= k is copied by whichever kernel owns it.  When the lengths kernel raised the
// flag, the later kernels return at once: only a row_ptr whose every row passed the check is used
// for addresses, and then the scan's total is at most nnz.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <type_traits>

#include "ofx_internal.h"
#include "row_topk.h"
#include "spmm_common.h"
#include "spmm_plan.h"

namespace ofx {
namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr int kListGrid = 2048;   // blocks that walk a row list
constexpr int kHubSlots = 4;      // keys per thread and emission chunk of a hub row
constexpr int kHubChunk = kBlock * kHubSlots;

// Keys of 16 bits are held in 32-bit registers.
template <typename U>
using reg_t = std::conditional_t<sizeof(U) == 8, uint64_t, uint32_t>;

__device__ __forceinline__ uint64_t lanes_below() {
  return (1ull << (threadIdx.x & 63)) - 1ull;
}

template <typename I>
__global__ void __launch_bounds__(kBlock)
    topk_lengths_kernel(const I* __restrict__ row_ptr, int64_t m, int64_t nnz, int k,
                        I* __restrict__ out_rp, int* __restrict__ wide_list, int wide_cap,
                        int* __restrict__ hub_list, int hub_cap, int* __restrict__ counts,
                        unsigned int* __restrict__ bad) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i == 0) out_rp[0] = (I)0;
  int64_t deg = 0;
  if (i < m) {
    const int64_t lo = (int64_t)row_ptr[i], hi = (int64_t)row_ptr[i + 1];
    if (nsg::row_ok(lo, hi, nnz))
      deg = hi - lo;
    else
      *bad = 1u;  // every writer stores the same word; the row counts as empty
    out_rp[i + 1] = (I)(deg < (int64_t)k ? deg : (int64_t)k);
  }
  // one atomic per wave and class; the lists hold what a CSR can: more rows mean a bad row_ptr
  const bool cls[2] = {deg > rtk::kNarrowMax && deg <= rtk::kWaveMax, deg > rtk::kWaveMax};
  int* const list[2] = {wide_list, hub_list};
  const int cap[2] = {wide_cap, hub_cap};
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    const uint64_t mask = __ballot(cls[c]);
    if (mask == 0ull) continue;
    int base = 0;
    if ((threadIdx.x & 63) == __ffsll((unsigned long long)mask) - 1)
      base = atomicAdd(counts + c, __popcll(mask));
    base = __shfl(base, __ffsll((unsigned long long)mask) - 1);
    if (cls[c]) {
      const int slot = base + __popcll(mask & lanes_below());
      if (slot < cap[c])
        list[c][slot] = (int)i;
      else
        *bad = 1u;
    }
  }
}

template <int G>
__device__ __forceinline__ int group_sum(int c) {
#pragma unroll
  for (int off = G / 2; off > 0; off >>= 1) c += __shfl_xor(c, off);
  return c;
}

template <typename I, typename U, int G, bool LIST>
__global__ void __launch_bounds__(kBlock)
    topk_group_kernel(const I* __restrict__ row_ptr, const I* __restrict__ col_idx,
                      const U* __restrict__ values, int64_t m, int k, U flip,
                      const int* __restrict__ list, const int* __restrict__ list_count,
                      int list_cap, const I* __restrict__ rp_s, I* __restrict__ out_col,
                      I* __restrict__ out_eid, int64_t* __restrict__ out_nnz,
                      const unsigned int* __restrict__ bad) {
  using K = reg_t<U>;
  constexpr int R = rtk::kSlots;
  constexpr int kBits = 8 * (int)sizeof(U);
  constexpr int kGroupsPerWave = 64 / G;
  constexpr uint64_t kGroupMask = G == 64 ? ~0ull : ((1ull << (G & 63)) - 1ull);
  const int t = (int)(threadIdx.x & (G - 1));
  const int group_base = (int)(threadIdx.x & 63 & ~(G - 1));
  if (!LIST && blockIdx.x == 0 && threadIdx.x == 0) *out_nnz = (int64_t)rp_s[m];
  if (*bad != 0u) return;
  int64_t count = m;
  if (LIST) {
    const int n = *list_count;
    count = n < list_cap ? n : list_cap;
  }
  const int64_t stride = (int64_t)gridDim.x * (kBlock / G);
  const int64_t wave_first =
      ((int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6)) * kGroupsPerWave;
  // The trip count is the wave's: every lane stays for the cross-lane steps.
  for (int64_t first = wave_first; first < count; first += stride) {
    const int64_t idx = first + group_base / G;
    int64_t begin = 0, o = 0;
    int deg = 0;
    if (idx < count) {
      const int64_t row = LIST ? (int64_t)list[idx] : idx;
      begin = (int64_t)row_ptr[row];
      const int64_t d = (int64_t)row_ptr[row + 1] - begin;
      deg = d <= (int64_t)(G * R) ? (int)d : 0;  // a longer row is on a list
      o = (int64_t)rp_s[row];
    }
    int ns = (deg + G - 1) / G;
#pragma unroll
    for (int off = 32; off >= G; off >>= 1) {
      const int other = __shfl_xor(ns, off);
      ns = other > ns ? other : ns;
    }
    ns = __builtin_amdgcn_readfirstlane(ns);  // the slots any group of the wave uses

    K key[R];
    uint32_t valid = 0u;
#pragma unroll
    for (int s = 0; s < R; ++s) {
      key[s] = (K)0;
      const int p = s * G + t;
      if (s < ns && p < deg) {
        key[s] = (K)rtk::key_of<U>(values[begin + p], flip);
        valid |= 1u << s;
      }
    }
    const bool selecting = deg > k;
    uint32_t cand = selecting ? valid : 0u;  // slots still undecided
    uint32_t sel = selecting ? 0u : valid;   // slots kept for certain
    int want = selecting ? k : 0;            // how many of the candidates are kept
    int ncand = selecting ? deg : 0;
    if (__ballot(selecting) != 0ull) {
      for (int b = kBits - 1; b >= 0; --b) {
        uint32_t hit = 0u;
#pragma unroll
        for (int s = 0; s < R; ++s)
          if (s < ns) hit |= (uint32_t)((key[s] >> b) & (K)1) << s;
        hit &= cand;
        const int c = group_sum<G>(__popc(hit));
        if (c >= want) {
          cand = hit;
          ncand = c;
        } else {
          sel |= hit;
          cand &= ~hit;
          want -= c;
          ncand -= c;
        }
        if (ncand == want) {  // every candidate is kept
          sel |= cand;
          cand = 0u;
          want = 0;
          ncand = 0;
        }
        if (__ballot(ncand != 0) == 0ull) break;
      }
    }
    // The candidates left hold one key: the first `want` by position are kept.  Position order is
    // slot by slot, lane by lane, for the ties and for the output alike.
    int tie_run = 0, out_run = 0;
#pragma unroll
    for (int s = 0; s < R; ++s) {
      if (s >= ns) break;
      const bool tie = ((cand >> s) & 1u) != 0u;
      const uint64_t tb = (__ballot(tie) >> group_base) & kGroupMask;
      const int tie_rank = tie_run + __popcll(tb & (((uint64_t)1 << t) - 1ull));
      tie_run += __popcll(tb);
      const bool keep = ((sel >> s) & 1u) != 0u || (tie && tie_rank < want);
      const uint64_t kb = (__ballot(keep) >> group_base) & kGroupMask;
      if (keep) {
        const int64_t e = begin + s * G + t;
        const int64_t at = o + out_run + __popcll(kb & (((uint64_t)1 << t) - 1ull));
        out_col[at] = col_idx[e];
        if (out_eid != nullptr) out_eid[at] = (I)e;
      }
      out_run += __popcll(kb);
    }
  }
}

template <typename I, typename U>
__global__ void __launch_bounds__(kBlock)
    topk_hub_kernel(const I* __restrict__ row_ptr, const I* __restrict__ col_idx,
                    const U* __restrict__ values, int k, U flip, const int* __restrict__ list,
                    const int* __restrict__ list_count, int list_cap, const I* __restrict__ rp_s,
                    I* __restrict__ out_col, I* __restrict__ out_eid,
                    const unsigned int* __restrict__ bad) {
  using K = reg_t<U>;
  constexpr int kBits = 8 * (int)sizeof(U);
  __shared__ int hist[256];
  __shared__ int wave_sum[kWaves];
  __shared__ int pick[3];  // the digit, the count still wanted, the digit's bin
  __shared__ int table[2][kHubSlots * kWaves * 2];
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (*bad != 0u) return;
  const int n = *list_count < list_cap ? *list_count : list_cap;
  for (int idx = (int)blockIdx.x; idx < n; idx += (int)gridDim.x) {  // the block's trip count
    const int64_t row = (int64_t)list[idx];
    const int64_t begin = (int64_t)row_ptr[row];
    const int deg = (int)((int64_t)row_ptr[row + 1] - begin);
    const int64_t o = (int64_t)rp_s[row];
    if (deg <= k) {
      for (int p = tid; p < deg; p += kBlock) {
        out_col[o + p] = col_idx[begin + p];
        if (out_eid != nullptr) out_eid[o + p] = (I)(begin + p);
      }
      continue;
    }
    // Select: after a pass, `prefix` is the top (kBits - shift) bits of the k-th largest key and
    // `want` how many keys with exactly that prefix are kept.
    K prefix = (K)0;
    int want = k, shift = kBits;
    for (int pass = 0; pass < kBits / 8; ++pass) {
      shift -= 8;
      hist[tid] = 0;
      __syncthreads();
      for (int p = tid; p < deg; p += kBlock) {
        const K key = (K)rtk::key_of<U>(values[begin + p], flip);
        if (pass == 0 || (key >> (shift + 8)) == prefix)
          atomicAdd(&hist[(int)((key >> shift) & (K)255)], 1);
      }
      __syncthreads();
      const int h = hist[tid];
      int above = h;  // bins tid..255, inclusive
#pragma unroll
      for (int off = 1; off < 64; off <<= 1) {
        const int v = __shfl_down(above, off);
        if (lane + off < 64) above += v;
      }
      if (lane == 0) wave_sum[wave] = above;
      __syncthreads();
      for (int w = wave + 1; w < kWaves; ++w) above += wave_sum[w];
      if (above >= want && above - h < want) {  // exactly one bin
        pick[0] = tid;
        pick[1] = want - (above - h);
        pick[2] = h;
      }
      __syncthreads();
      prefix = (K)((prefix << 8) | (K)pick[0]);
      want = pick[1];
      if (pick[2] == want) break;  // the whole bin is kept: the lower bits decide nothing
    }
    // Emit: keys above the prefix at `shift`, and the first `want` of those equal to it.
    int gt_base = 0, eq_base = 0;
    for (int c0 = 0, par = 0; c0 < deg; c0 += kHubChunk, par ^= 1) {
      int gt_below[kHubSlots], eq_below[kHubSlots];
      uint32_t gt = 0u, eq = 0u;
#pragma unroll
      for (int r = 0; r < kHubSlots; ++r) {
        const int p = c0 + r * kBlock + tid;
        bool g = false, e = false;
        if (p < deg) {
          const K top = (K)rtk::key_of<U>(values[begin + p], flip) >> shift;
          g = top > prefix;
          e = top == prefix;
        }
        const uint64_t bg = __ballot(g), be = __ballot(e);
        if (lane == 0) {
          table[par][(r * kWaves + wave) * 2] = __popcll(bg);
          table[par][(r * kWaves + wave) * 2 + 1] = __popcll(be);
        }
        gt_below[r] = __popcll(bg & lanes_below());
        eq_below[r] = __popcll(be & lanes_below());
        gt |= (uint32_t)g << r;
        eq |= (uint32_t)e << r;
      }
      __syncthreads();  // one per chunk: the table alternates, so the next chunk's writes wait
      int run_g = gt_base, run_e = eq_base;
#pragma unroll
      for (int r = 0; r < kHubSlots; ++r) {
#pragma unroll
        for (int w = 0; w < kWaves; ++w) {
          if (w == wave) {
            const int eq_before = run_e + eq_below[r];
            const bool keep = ((gt >> r) & 1u) != 0u || (((eq >> r) & 1u) != 0u && eq_before < want);
            if (keep) {
              const int64_t e = begin + c0 + r * kBlock + tid;
              const int64_t at =
                  o + run_g + gt_below[r] + (eq_before < want ? eq_before : want);
              out_col[at] = col_idx[e];
              if (out_eid != nullptr) out_eid[at] = (I)e;
            }
          }
          run_g += table[par][(r * kWaves + w) * 2];
          run_e += table[par][(r * kWaves + w) * 2 + 1];
        }
      }
      gt_base = run_g;
      eq_base = run_e;
      if (gt_base + (eq_base < want ? eq_base : want) >= k) break;  // the row's k are out
    }
    __syncthreads();  // the next row's first chunk may use either half of the table
  }
}

// The workspace: a function of (idx_dtype, m, nnz) alone.  Every part is aligned to 256 bytes.
struct TopkWs {
  size_t head, wide, hub, cub, cub_bytes, total;  // head: the flag, then the two list counts
  int wide_cap, hub_cap;
};

int topk_ws(int idx_dtype, int64_t m, int64_t nnz, TopkWs* w) {
  *w = TopkWs{};
  if (m != 0) {
    const int rc = by_index(idx_dtype, [&](auto* ip) -> int {
      using I = std::remove_pointer_t<decltype(ip)>;
      OFX_HIP_CHECK(hipcub::DeviceScan::InclusiveSum(nullptr, w->cub_bytes, (I*)nullptr,
                                                     (I*)nullptr, (int)m));
      return OFX_OK;
    });
    if (rc) return rc;
  }
  const int64_t wide = nnz / (rtk::kNarrowMax + 1), hub = nnz / (rtk::kWaveMax + 1);
  w->wide_cap = (int)(wide < m ? wide : m);
  w->hub_cap = (int)(hub < m ? hub : m);
  size_t off = 256;
  w->wide = off;
  off = plan::align_up(off + (size_t)w->wide_cap * sizeof(int), 256);
  w->hub = off;
  off = plan::align_up(off + (size_t)w->hub_cap * sizeof(int), 256);
  w->cub = off;
  w->total = plan::align_up(off + w->cub_bytes, 256);
  return OFX_OK;
}

template <typename I, typename U>
int topk(hipStream_t s, int64_t m, int64_t nnz, const I* rp, const I* ci, const U* values, int k,
         U flip, I* out_rp, I* out_col, I* out_eid, int64_t* out_nnz, unsigned int* bad_out,
         char* ws, size_t ws_bytes) {
  if (bad_out) OFX_HIP_CHECK(hipMemsetAsync(bad_out, 0, sizeof(unsigned int), s));
  if (m == 0) {
    OFX_HIP_CHECK(hipMemsetAsync(out_rp, 0, sizeof(I), s));
    OFX_HIP_CHECK(hipMemsetAsync(out_nnz, 0, sizeof(int64_t), s));
    return OFX_OK;
  }
  TopkWs w;
  const int rc = topk_ws(sizeof(I) == 4 ? OFX_DT_INT32 : OFX_DT_INT64, m, nnz, &w);
  if (rc) return rc;
  OFX_REQUIRE(ws && ws_bytes >= w.total, OFX_EWORKSPACE,
              "row_topk: workspace of %zu bytes < %zu required", ws_bytes, w.total);
  auto* head = reinterpret_cast<unsigned int*>(ws + w.head);
  auto* bad = bad_out ? bad_out : head;
  int* counts = reinterpret_cast<int*>(head + 1);
  int* wide_list = reinterpret_cast<int*>(ws + w.wide);
  int* hub_list = reinterpret_cast<int*>(ws + w.hub);
  OFX_HIP_CHECK(hipMemsetAsync(head, 0, 3 * sizeof(unsigned int), s));
  const unsigned row_blocks = (unsigned)((m + kBlock - 1) / kBlock);
  hipLaunchKernelGGL((topk_lengths_kernel<I>), dim3(row_blocks), dim3(kBlock), 0, s, rp, m, nnz, k,
                     out_rp, wide_list, w.wide_cap, hub_list, w.hub_cap, counts, bad);
  OFX_HIP_CHECK(hipGetLastError());
  size_t cb = w.cub_bytes;
  OFX_HIP_CHECK(hipcub::DeviceScan::InclusiveSum(ws + w.cub, cb, out_rp + 1, out_rp + 1, (int)m, s));
  // every row, eight to a wave; the rows of more than 64 entries are left to the lists
  const int64_t narrow_blocks = (m * rtk::kNarrowGroup + kBlock - 1) / kBlock;
  hipLaunchKernelGGL((topk_group_kernel<I, U, rtk::kNarrowGroup, false>),
                     dim3((unsigned)narrow_blocks), dim3(kBlock), 0, s, rp, ci, values, m, k, flip,
                     nullptr, nullptr, 0, out_rp, out_col, out_eid, out_nnz, bad);
  OFX_HIP_CHECK(hipGetLastError());
  if (w.wide_cap != 0) {
    const int blocks = (w.wide_cap + kWaves - 1) / kWaves;
    hipLaunchKernelGGL((topk_group_kernel<I, U, 64, true>),
                       dim3((unsigned)(blocks < kListGrid ? blocks : kListGrid)), dim3(kBlock), 0, s,
                       rp, ci, values, m, k, flip, wide_list, counts, w.wide_cap, out_rp, out_col,
                       out_eid, out_nnz, bad);
    OFX_HIP_CHECK(hipGetLastError());
  }
  if (w.hub_cap != 0) {
    hipLaunchKernelGGL((topk_hub_kernel<I, U>),
                       dim3((unsigned)(w.hub_cap < kListGrid ? w.hub_cap : kListGrid)), dim3(kBlock),
                       0, s, rp, ci, values, k, flip, hub_list, counts + 1, w.hub_cap, out_rp,
                       out_col, out_eid, bad);
    OFX_HIP_CHECK(hipGetLastError());
  }
  return OFX_OK;
}

}  // namespace
}  // namespace ofx

using namespace ofx;

extern "C" int ofx_row_topk_workspace_size(int idx_dtype, int64_t m, int64_t nnz, size_t* bytes) {
  return ::ofx::guarded(__func__, [&]() -> int {
    OFX_REQUIRE(bytes, OFX_EINVAL, "row_topk: NULL pointer");
    const int rc = rtk::check_topk_sizes("row_topk", idx_dtype, m, nnz);
    if (rc) return rc;
    TopkWs w;
    const int rw = topk_ws(idx_dtype, m, nnz, &w);
    *bytes = w.total;
    return rw;
  });
}

extern "C" int ofx_row_topk(void* stream, int idx_dtype, int val_dtype, int64_t m, int64_t nnz,
                            const void* row_ptr, const void* col_idx, const void* values, int64_t k,
                            int largest, void* out_row_ptr, void* out_col_idx, void* out_edge_ids,
                            void* out_nnz, void* bad_flag, void* workspace,
                            size_t workspace_bytes) {
  return ::ofx::guarded(__func__, [&]() -> int {
    const int rc = rtk::check_topk_args("row_topk", idx_dtype, val_dtype, m, nnz, row_ptr, col_idx,
                                        values, k, out_row_ptr, out_col_idx, out_nnz);
    if (rc) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int kk = rtk::clamp_k(k);
    return by_index(idx_dtype, [&](auto* ip) -> int {
      using I = std::remove_pointer_t<decltype(ip)>;
      return rtk::by_key(val_dtype, [&](auto* up) -> int {
        using U = std::remove_pointer_t<decltype(up)>;
        return topk<I, U>(s, m, nnz, (const I*)row_ptr, (const I*)col_idx, (const U*)values, kk,
                          largest ? (U)0 : (U)~(U)0, (I*)out_row_ptr, (I*)out_col_idx,
                          (I*)out_edge_ids, (int64_t*)out_nnz, (unsigned int*)bad_flag,
                          (char*)workspace, workspace_bytes);
      });
    });
  });
}
