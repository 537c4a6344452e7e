// spgemm.hip — CSR x CSR -> CSR on the device, gfx950 (contract in include/ofx_spmm.h, rules in
// spgemm.h).  A row-wise Gustavson product: every row of C is built in an
// open-addressing hash table in LDS by the group of lanes that owns the row; products never reach
// global memory, only the distinct columns (and their sums) do.
//
// count entry:
//   clear kernel   : the head of the workspace (flag, counters, list lengths).
//   B check        : one pass over B's rows (entry range) and one over B's entries (column in
//                    [0, n)).  Strict ascent without a search for the row of an entry: the entries
//                    j with col[j] <= col[j-1] are counted, and so are the starts of non-empty rows
//                    with col[start] <= col[start-1]; every descent stands at a row start exactly
//                    when the two counts agree.
//   bound kernel   : eight lanes per row of A: the row check, ub_i = sum of deg_b(col_a[p]) in
//                    int64, the row's class by ub_i and its place in that class's row list (one
//                    atomic per wave and class).  A row with ub_i = 0 is empty and is not listed.
//   row kernel     : the row template below, symbolic: the distinct columns of every listed row.
//   hipcub scan    : the row counts in int64 in the workspace (nnz_c may pass an int32 index).
//   finish kernel  : out_row_ptr from the scan, out_nnz, the flag.
// fill entry: the row kernel, numeric, over the same lists.
//
// The row template (one for both phases, a compile-time switch), for a group of G lanes and a
// table of TS = 2 * MAX slots, MAX the class's bound on ub:
//   insert     : lanes stride over B's row col_a[p]; linear probing from a multiplicative hash, an
//                LDS atomicCAS on the key; a new key counts.  The table is at most half full, and
//                every probe loop is bounded by TS.
//   (symbolic stops here: the count.)
//   compact    : the used slots' keys into a list, padded to a power of two.
//   sort       : bitonic, in LDS (rank by counting costs d^2 / G reads: 16 times more at d = 2048).
//   accumulate : p sequential and the same for the whole wave, lanes striding over B's row; a lane
//                finds its column's slot and does acc[slot] = acc[slot] + t, no atomic: B's row is
//                strictly ascending, so no two lanes of a step share a slot, and the steps of a wave
//                are in program order.  The accumulator is indexed by the slot, not by the rank: the
//                rank is needed only when the row is stored, and a rank array would cost the LDS
//                the accumulators of the empty half of the table do.
//   store      : the sorted columns, and for each its slot's sum rounded to the value type.
// G = 8 (eight rows a wave), 64 (a row a wave) and 256 (a row a block).  In the block every wave
// owns the columns of one residue class mod 4 and walks all of A's row itself, so a column's chain
// stays inside one wave and needs no barrier per step; the inserts, which have no order, split p
// among the waves instead.  (Rejected: p split among the waves with a barrier per step, one barrier
// per entry of A; and atomic adds, which lose the order.)
// Hub rows (ub > 2048) use the block form over column ranges [lo, hi): B's rows are ascending, so a
// wave-uniform binary search finds each row's first column at or above lo and the lanes stop at hi.
// The first range is all of [0, n); a range in which more than 2048 distinct columns turn up is
// abandoned and halved (a one-column range always fits; the decision is read from LDS after a
// barrier, so it is the block's).  Ranges come out ascending, so the row does too, and every column's
// chain is computed whole inside the range that holds it.  A block-class row is a hub row whose
// first range fits.
// Lanes of a group narrower than a wave rely on the wave executing its lanes in lockstep; the
// compiler is held to program order by a wavefront fence at every step.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <type_traits>

#include "ofx_internal.h"
#include "spgemm.h"
#include "spmm_common.h"
#include "spmm_plan.h"

namespace ofx {
namespace {

constexpr int kBlock = 256;
constexpr int kListGrid = 4096;  // blocks that walk a row list
constexpr int kEmpty = -1;       // no column is negative
constexpr int kBoundGroup = 8;   // lanes per row of A in the bound kernel

// The head of the workspace.
struct Head {
  unsigned int flag;       // spg::kBad* bits
  unsigned int descents;   // entries of B not above the entry before them
  unsigned int start_descents;  // of these, the ones at the start of a non-empty row
  int counts[spg::kClasses];    // the lengths of the row lists
};

__device__ __forceinline__ uint64_t lanes_below() {
  return (1ull << (threadIdx.x & 63)) - 1ull;
}

__device__ __forceinline__ bool stopped(const Head* head) {
  return head->flag != 0u || head->descents != head->start_descents;
}

__global__ void spgemm_clear_kernel(Head* head, int64_t* rowc) {
  if (threadIdx.x == 0) {
    *head = Head{};
    rowc[0] = 0;
  }
}

template <typename I>
__global__ void __launch_bounds__(kBlock)
    spgemm_check_b_kernel(const I* __restrict__ rp_b, const I* __restrict__ ci_b, int64_t k,
                          int64_t n, int64_t nnz_b, Head* __restrict__ head) {
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  const int64_t first_t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  // the entries the rows cover when every row is good: [first, last)
  int64_t first = (int64_t)rp_b[0], last = (int64_t)rp_b[k];
  first = first < 0 ? 0 : first > nnz_b ? nnz_b : first;
  last = last < first ? first : last > nnz_b ? nnz_b : last;
  bool outside = false;
  int desc = 0, start_desc = 0;
  for (int64_t r = first_t; r < k; r += stride) {
    const int64_t lo = (int64_t)rp_b[r], hi = (int64_t)rp_b[r + 1];
    if (!nsg::row_ok(lo, hi, nnz_b))
      outside = true;
    else if (lo < hi && lo > first && lo < last && (int64_t)ci_b[lo] <= (int64_t)ci_b[lo - 1])
      ++start_desc;
  }
  for (int64_t j = first + first_t; j < last; j += stride) {
    const int64_t c = (int64_t)ci_b[j];
    if (c < 0 || c >= n) outside = true;
    if (j > first && c <= (int64_t)ci_b[j - 1]) ++desc;
  }
  if (outside) head->flag = spg::kBadOutside;  // every writer stores the same word
  for (int off = 32; off > 0; off >>= 1) {
    desc += __shfl_xor(desc, off);
    start_desc += __shfl_xor(start_desc, off);
  }
  if ((threadIdx.x & 63) == 0) {
    if (desc != 0) atomicAdd(&head->descents, (unsigned int)desc);
    if (start_desc != 0) atomicAdd(&head->start_descents, (unsigned int)start_desc);
  }
}

template <typename I>
__global__ void __launch_bounds__(kBlock)
    spgemm_bound_kernel(const I* __restrict__ rp_a, const I* __restrict__ ci_a,
                        const I* __restrict__ rp_b, int64_t m, int64_t k, int64_t nnz_a,
                        int64_t nnz_b, int64_t* __restrict__ rowc, int* __restrict__ lists,
                        int64_t list_stride, int list_cap, Head* __restrict__ head) {
  constexpr int G = kBoundGroup;
  const int t = (int)(threadIdx.x & (G - 1));
  const int64_t i = ((int64_t)blockIdx.x * kBlock + threadIdx.x) / G;
  int64_t ub = 0;
  bool outside = false;
  if (i < m) {
    const int64_t lo = (int64_t)rp_a[i], hi = (int64_t)rp_a[i + 1];
    if (!nsg::row_ok(lo, hi, nnz_a)) {
      outside = true;
    } else {
      for (int64_t p = lo + t; p < hi; p += G) {
        const int64_t c = (int64_t)ci_a[p];
        if (c < 0) outside = true;
        if (c < 0 || c >= k) continue;  // at or above k: a zero row
        const int64_t blo = (int64_t)rp_b[c], bhi = (int64_t)rp_b[c + 1];
        if (nsg::row_ok(blo, bhi, nnz_b)) ub += bhi - blo;  // a bad row: the B check's flag
      }
    }
  }
  if (outside) head->flag = spg::kBadOutside;
#pragma unroll
  for (int off = G / 2; off > 0; off >>= 1) ub += __shfl_xor(ub, off);
  const bool leader = t == 0 && i < m;
  if (leader && ub == 0) rowc[i + 1] = 0;
  const int cls = spg::class_of(ub);
#pragma unroll
  for (int c = 0; c < spg::kClasses; ++c) {
    const bool mine = leader && ub != 0 && cls == c;
    const uint64_t mask = __ballot(mine);
    if (mask == 0ull) continue;
    const int first = __ffsll((unsigned long long)mask) - 1;
    int base = 0;
    if ((int)(threadIdx.x & 63) == first) base = atomicAdd(&head->counts[c], __popcll(mask));
    base = __shfl(base, first);
    if (mine) {
      const int slot = base + __popcll(mask & lanes_below());
      if (slot < list_cap)
        lists[c * list_stride + slot] = (int)i;
      else
        head->flag = spg::kBadOutside;  // more listed rows than a CSR of these sizes has
    }
  }
}

// ---- the row template ---------------------------------------------------------------------------
template <int G>
__device__ __forceinline__ void group_sync() {
  if constexpr (G > 64) {
    __syncthreads();
  } else {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
  }
}

template <int TS>
__device__ __forceinline__ int slot_of(int c) {
  constexpr int kLog = __builtin_ctz((unsigned)TS);
  return (int)(((uint32_t)c * 2654435761u) >> (32 - kLog));
}

// 1: a new key, 0: present already (or, on a table that is full, which no class allows, dropped).
template <int TS>
__device__ __forceinline__ int table_insert(int* keys, int c) {
  int s = slot_of<TS>(c);
  for (int probe = 0; probe < TS; ++probe) {
    const int old = atomicCAS(&keys[s], kEmpty, c);
    if (old == kEmpty) return 1;
    if (old == c) return 0;
    s = (s + 1) & (TS - 1);
  }
  return 0;
}

// The slot of a key that is present, or -1.
template <int TS>
__device__ __forceinline__ int table_find(const int* keys, int c) {
  int s = slot_of<TS>(c);
  for (int probe = 0; probe < TS; ++probe) {
    const int key = keys[s];
    if (key == c) return s;
    if (key == kEmpty) return -1;
    s = (s + 1) & (TS - 1);
  }
  return -1;
}

// The first entry of [b0, b1) whose column is at or above lo; the row is ascending.
template <typename I>
__device__ __forceinline__ int64_t lower_bound(const I* __restrict__ ci, int64_t b0, int64_t b1,
                                               int64_t lo) {
  while (b0 < b1) {
    const int64_t mid = b0 + ((b1 - b0) >> 1);
    if ((int64_t)ci[mid] < lo)
      b0 = mid + 1;
    else
      b1 = mid;
  }
  return b0;
}

// The products of A's entries p = a0 + first, a0 + first + step, ... with B's rows, columns in
// [lo, hi): W lanes stride over a row of B and call f(p, q, column).  `quit`, when given, is an LDS
// word that ends the walk once it is set.
template <typename I, int W, typename F>
__device__ __forceinline__ void walk(const I* __restrict__ ci_a, const I* __restrict__ rp_b,
                                     const I* __restrict__ ci_b, int64_t a0, int64_t a1, int first,
                                     int step, int lane, int64_t k, int64_t lo, int64_t hi,
                                     const volatile int* quit, F&& f) {
  for (int64_t p = a0 + first; p < a1; p += step) {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");  // a step after the step before it
    __builtin_amdgcn_wave_barrier();
    if (quit != nullptr && *quit != 0) break;
    const int64_t ca = (int64_t)ci_a[p];
    if (ca < 0 || ca >= k) continue;
    int64_t b0 = (int64_t)rp_b[ca];
    const int64_t b1 = (int64_t)rp_b[ca + 1];
    if (lo > 0) b0 = lower_bound(ci_b, b0, b1, lo);
    for (int64_t q = b0 + lane; q < b1; q += W) {
      const int64_t c = (int64_t)ci_b[q];
      if (c >= hi) break;
      f(p, q, (int)c);
    }
  }
}

template <typename I, typename T, int G, bool NUMERIC>
__global__ void __launch_bounds__(kBlock)
    spgemm_rows_kernel(const I* __restrict__ rp_a, const I* __restrict__ ci_a,
                       const T* __restrict__ va, const I* __restrict__ rp_b,
                       const I* __restrict__ ci_b, const T* __restrict__ vb, int64_t k, int64_t n,
                       const int* __restrict__ list, const int* __restrict__ list_count,
                       int list_cap, const Head* __restrict__ head, int64_t* __restrict__ rowc,
                       const I* __restrict__ rp_c, I* __restrict__ out_col,
                       T* __restrict__ out_val) {
  using Acc = typename Num<T>::acc;
  constexpr int MAX = G == 8 ? spg::kNarrowMax : G == 64 ? spg::kWaveMax : spg::kBlockMax;
  constexpr int TS = 2 * MAX;
  constexpr int GROUPS = kBlock / G;
  constexpr int W = G < 64 ? G : 64;  // the lanes that stride over one row of B
  constexpr int SUB = G / W;          // the waves of a block group
  __shared__ int s_keys[GROUPS * TS];
  __shared__ int s_cnt[GROUPS * 2];  // the distinct columns; overflow, then the compaction's cursor
  __shared__ Acc s_acc[NUMERIC ? GROUPS * TS : 1];
  __shared__ int s_cols[NUMERIC ? GROUPS * MAX : 1];
  const int g = (int)threadIdx.x / G, t = (int)threadIdx.x % G;
  const int lane = t % W, sub = t / W;
  int* const keys = s_keys + g * TS;
  int* const cnt = s_cnt + g * 2;
  Acc* const acc = s_acc + (NUMERIC ? g * TS : 0);
  int* const cols = s_cols + (NUMERIC ? g * MAX : 0);
  if (stopped(head)) return;
  const int listed = *list_count < list_cap ? *list_count : list_cap;
  // G = 256: the trip counts of both loops are the block's.
  for (int64_t idx = (int64_t)blockIdx.x * GROUPS + g; idx < listed;
       idx += (int64_t)gridDim.x * GROUPS) {
    const int64_t row = (int64_t)list[idx];
    const int64_t a0 = (int64_t)rp_a[row], a1 = (int64_t)rp_a[row + 1];
    int64_t o = 0, o_end = 0, total = 0;
    if (NUMERIC) {
      o = (int64_t)rp_c[row];
      o_end = (int64_t)rp_c[row + 1];
    }
    int64_t lo = 0, width = n;
    while (lo < n) {
      const int64_t hi = lo + width < n ? lo + width : n;
      for (int s = t; s < TS; s += G) {
        keys[s] = kEmpty;
        if (NUMERIC) acc[s] = Acc(0);
      }
      if (t == 0) cnt[0] = cnt[1] = 0;
      group_sync<G>();
      // insert: no order is needed, so the waves of a block split p
      walk<I, W>(ci_a, rp_b, ci_b, a0, a1, sub, SUB, lane, k, lo, hi,
                 G > 64 ? (const volatile int*)(cnt + 1) : nullptr, [&](int64_t, int64_t, int c) {
                   if (G > 64 && *(const volatile int*)(cnt + 1) != 0) return;  // abandoned
                   if (table_insert<TS>(keys, c) != 0 && atomicAdd(&cnt[0], 1) >= MAX) cnt[1] = 1;
                 });
      group_sync<G>();
      const int d = cnt[0];
      const bool over = G > 64 && cnt[1] != 0;
      group_sync<G>();
      if (over) {  // only ub > MAX gets here, and a one-column range holds one column
        width = (width + 1) >> 1;
        continue;
      }
      if (NUMERIC) {
        for (int s = t; s < TS; s += G) {
          const int key = keys[s];
          if (key != kEmpty) {
            const int at = atomicAdd(&cnt[1], 1);
            if (at < MAX) cols[at] = key;
          }
        }
        int pow2 = 1;
        while (pow2 < d) pow2 <<= 1;
        pow2 = pow2 < MAX ? pow2 : MAX;
        for (int r = d + t; r < pow2; r += G) cols[r] = INT_MAX;
        group_sync<G>();
        for (int span = 2; span <= pow2; span <<= 1) {
          for (int j = span >> 1; j > 0; j >>= 1) {
            for (int r = t; r < pow2; r += G) {
              const int other = r ^ j;
              if (other > r) {
                const int x = cols[r], y = cols[other];
                if ((x > y) == ((r & span) == 0)) {
                  cols[r] = y;
                  cols[other] = x;
                }
              }
            }
            group_sync<G>();
          }
        }
        if (out_val != nullptr) {
          // every wave walks all of A's row in order and keeps to its own columns
          walk<I, W>(ci_a, rp_b, ci_b, a0, a1, 0, 1, lane, k, lo, hi, nullptr,
                     [&](int64_t p, int64_t q, int c) {
                       if (SUB > 1 && (c & (SUB - 1)) != sub) return;
                       const int s = table_find<TS>(keys, c);
                       if (s >= 0)
                         acc[s] = acc[s] + Acc(Num<T>::mul(Num<T>::load(va[p]), Num<T>::load(vb[q])));
                     });
          group_sync<G>();
        }
        const int dn = d < MAX ? d : MAX;
        for (int r = t; r < dn && o + r < o_end; r += G) {
          const int c = cols[r];
          out_col[o + r] = (I)c;
          if (out_val != nullptr) {
            const int s = table_find<TS>(keys, c);
            out_val[o + r] = Num<T>::store(s >= 0 ? acc[s] : Acc(0));
          }
        }
        o += d;
        group_sync<G>();
      }
      total += d;
      lo = hi;
    }
    if (!NUMERIC && t == 0) rowc[row + 1] = total;
  }
}

template <typename I>
__global__ void __launch_bounds__(kBlock)
    spgemm_finish_kernel(const int64_t* __restrict__ rowc, int64_t m, I* __restrict__ out_rp,
                         int64_t* __restrict__ out_nnz, Head* __restrict__ head,
                         unsigned int* __restrict__ bad_out) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const bool stop = stopped(head);
  if (i <= m) out_rp[i] = stop ? (I)0 : (I)rowc[i];
  if (i == 0) {
    unsigned int flag = head->flag;
    if (head->descents != head->start_descents) flag |= spg::kBadAscending;
    if (bad_out != nullptr) *bad_out = flag;
    *out_nnz = stop ? 0 : rowc[m];
  }
}

// The workspace: a function of (m, nnz_a) alone.  Every part is aligned to 256 bytes.
struct SpgemmWs {
  size_t head, rowc, lists, cub, cub_bytes, total;
  int64_t list_stride;  // ints between two lists
  int list_cap;         // a listed row holds an entry of A
};

int spgemm_ws(int64_t m, int64_t nnz_a, SpgemmWs* w) {
  *w = SpgemmWs{};
  if (m != 0)
    OFX_HIP_CHECK(hipcub::DeviceScan::InclusiveSum(nullptr, w->cub_bytes, (int64_t*)nullptr,
                                                   (int64_t*)nullptr, (int)m));
  w->list_cap = (int)(nnz_a < m ? nnz_a : m);
  w->list_stride = (int64_t)plan::align_up((size_t)w->list_cap * sizeof(int), 256) / sizeof(int);
  size_t off = 256;
  w->rowc = off;
  off = plan::align_up(off + ((size_t)m + 1) * sizeof(int64_t), 256);
  w->lists = off;
  off = plan::align_up(off + (size_t)w->list_stride * sizeof(int) * spg::kClasses, 256);
  w->cub = off;
  w->total = plan::align_up(off + w->cub_bytes, 256);
  return OFX_OK;
}

int check_ws(const char* fn, int64_t m, int64_t nnz_a, const void* ws, size_t ws_bytes,
             SpgemmWs* w) {
  const int rc = spgemm_ws(m, nnz_a, w);
  if (rc) return rc;
  OFX_REQUIRE(ws && ws_bytes >= w->total, OFX_EWORKSPACE,
              "%s: workspace of %zu bytes < %zu required", fn, ws_bytes, w->total);
  OFX_REQUIRE(((uintptr_t)ws & 15u) == 0, OFX_EWORKSPACE,
              "%s: the workspace must be 16-byte aligned", fn);
  return OFX_OK;
}

unsigned grid_of(int64_t items, int per_block, int64_t cap) {
  const int64_t g = (items + per_block - 1) / per_block;
  return (unsigned)(g < 1 ? 1 : g > cap ? cap : g);
}

// The row kernel over the four lists, the longest rows first.
template <typename I, typename T, bool NUMERIC>
int launch_rows(hipStream_t s, int64_t k, int64_t n, const I* rp_a, const I* ci_a, const T* va,
                const I* rp_b, const I* ci_b, const T* vb, const I* rp_c, I* out_col, T* out_val,
                char* ws, const SpgemmWs& w) {
  auto* head = reinterpret_cast<Head*>(ws + w.head);
  auto* rowc = reinterpret_cast<int64_t*>(ws + w.rowc);
  const int* lists = reinterpret_cast<const int*>(ws + w.lists);
  for (int c = spg::kClasses - 1; c >= 0; --c) {
    const int cap = w.list_cap;
    if (cap == 0) continue;
    const int* list = lists + c * w.list_stride;
    const int* count = head->counts + c;  // an address, not a read
    if (c == 0) {
      hipLaunchKernelGGL((spgemm_rows_kernel<I, T, 8, NUMERIC>), dim3(grid_of(cap, kBlock / 8, kListGrid)),
                         dim3(kBlock), 0, s, rp_a, ci_a, va, rp_b, ci_b, vb, k, n, list, count, cap,
                         head, rowc, rp_c, out_col, out_val);
    } else if (c == 1) {
      hipLaunchKernelGGL((spgemm_rows_kernel<I, T, 64, NUMERIC>), dim3(grid_of(cap, kBlock / 64, kListGrid)),
                         dim3(kBlock), 0, s, rp_a, ci_a, va, rp_b, ci_b, vb, k, n, list, count, cap,
                         head, rowc, rp_c, out_col, out_val);
    } else {
      hipLaunchKernelGGL((spgemm_rows_kernel<I, T, 256, NUMERIC>), dim3(grid_of(cap, 1, kListGrid)),
                         dim3(kBlock), 0, s, rp_a, ci_a, va, rp_b, ci_b, vb, k, n, list, count, cap,
                         head, rowc, rp_c, out_col, out_val);
    }
    OFX_HIP_CHECK(hipGetLastError());
  }
  return OFX_OK;
}

template <typename I>
int count_phase(hipStream_t s, int64_t m, int64_t k, int64_t n, int64_t nnz_a, int64_t nnz_b,
                const I* rp_a, const I* ci_a, const I* rp_b, const I* ci_b, I* out_rp,
                int64_t* out_nnz, unsigned int* bad_out, char* ws, const SpgemmWs& w) {
  auto* head = reinterpret_cast<Head*>(ws + w.head);
  auto* rowc = reinterpret_cast<int64_t*>(ws + w.rowc);
  hipLaunchKernelGGL(spgemm_clear_kernel, dim3(1), dim3(64), 0, s, head, rowc);
  OFX_HIP_CHECK(hipGetLastError());
  const int64_t b_items = k > nnz_b ? k : nnz_b;
  hipLaunchKernelGGL((spgemm_check_b_kernel<I>), dim3(grid_of(b_items, kBlock, 8192)), dim3(kBlock),
                     0, s, rp_b, ci_b, k, n, nnz_b, head);
  OFX_HIP_CHECK(hipGetLastError());
  if (m != 0) {
    hipLaunchKernelGGL((spgemm_bound_kernel<I>), dim3(grid_of(m, kBlock / kBoundGroup, INT32_MAX)),
                       dim3(kBlock), 0, s, rp_a, ci_a, rp_b, m, k, nnz_a, nnz_b, rowc,
                       reinterpret_cast<int*>(ws + w.lists), w.list_stride, w.list_cap, head);
    OFX_HIP_CHECK(hipGetLastError());
    const int rc = launch_rows<I, float, false>(s, k, n, rp_a, ci_a, nullptr, rp_b, ci_b, nullptr,
                                                nullptr, nullptr, nullptr, ws, w);
    if (rc) return rc;
    size_t cb = w.cub_bytes;
    OFX_HIP_CHECK(hipcub::DeviceScan::InclusiveSum(ws + w.cub, cb, rowc + 1, rowc + 1, (int)m, s));
  }
  hipLaunchKernelGGL((spgemm_finish_kernel<I>), dim3(grid_of(m + 1, kBlock, INT32_MAX)),
                     dim3(kBlock), 0, s, rowc, m, out_rp, out_nnz, head, bad_out);
  OFX_HIP_CHECK(hipGetLastError());
  return OFX_OK;
}

}  // namespace
}  // namespace ofx

using namespace ofx;

extern "C" int ofx_spgemm_workspace_size(int idx_dtype, int val_dtype, int64_t m, int64_t k,
                                         int64_t n, int64_t nnz_a, int64_t nnz_b, size_t* bytes) {
  return ::ofx::guarded(__func__, [&]() -> int {
    OFX_REQUIRE(bytes, OFX_EINVAL, "spgemm: NULL pointer");
    const int rc = spg::check_spgemm_sizes("spgemm", idx_dtype, m, k, n, nnz_a, nnz_b);
    if (rc) return rc;
    OFX_REQUIRE(is_value_dtype(val_dtype), OFX_EUNSUPPORTED,
                "spgemm: value dtype %d is not float/double/float16/bfloat16", val_dtype);
    SpgemmWs w;
    const int rw = spgemm_ws(m, nnz_a, &w);
    *bytes = w.total;
    return rw;
  });
}

extern "C" int ofx_spgemm_count(void* stream, int idx_dtype, int64_t m, int64_t k, int64_t n,
                                int64_t nnz_a, int64_t nnz_b, const void* rp_a, const void* ci_a,
                                const void* rp_b, const void* ci_b, void* out_row_ptr,
                                void* out_nnz, void* bad_flag, void* workspace,
                                size_t workspace_bytes) {
  return ::ofx::guarded(__func__, [&]() -> int {
    const int rc = spg::check_count_args("spgemm_count", idx_dtype, m, k, n, nnz_a, nnz_b, rp_a,
                                         ci_a, rp_b, ci_b, out_row_ptr, out_nnz);
    if (rc) return rc;
    SpgemmWs w;
    const int rs = check_ws("spgemm_count", m, nnz_a, workspace, workspace_bytes, &w);
    if (rs) return rs;
    hipStream_t s = static_cast<hipStream_t>(stream);
    return by_index(idx_dtype, [&](auto* ip) -> int {
      using I = std::remove_pointer_t<decltype(ip)>;
      return count_phase<I>(s, m, k, n, nnz_a, nnz_b, (const I*)rp_a, (const I*)ci_a,
                            (const I*)rp_b, (const I*)ci_b, (I*)out_row_ptr, (int64_t*)out_nnz,
                            (unsigned int*)bad_flag, (char*)workspace, w);
    });
  });
}

extern "C" int ofx_spgemm_fill(void* stream, int idx_dtype, int val_dtype, int64_t m, int64_t k,
                               int64_t n, int64_t nnz_a, int64_t nnz_b, int64_t nnz_c,
                               const void* rp_a, const void* ci_a, const void* va, const void* rp_b,
                               const void* ci_b, const void* vb, const void* row_ptr_c,
                               void* out_col_idx, void* out_values, void* workspace,
                               size_t workspace_bytes) {
  return ::ofx::guarded(__func__, [&]() -> int {
    const int rc = spg::check_fill_args("spgemm_fill", idx_dtype, val_dtype, m, k, n, nnz_a, nnz_b,
                                        nnz_c, rp_a, ci_a, va, rp_b, ci_b, vb, row_ptr_c,
                                        out_col_idx, out_values);
    if (rc) return rc;
    SpgemmWs w;
    const int rs = check_ws("spgemm_fill", m, nnz_a, workspace, workspace_bytes, &w);
    if (rs) return rs;
    if (m == 0 || nnz_c == 0) return OFX_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    // pattern only: the float instantiation, which reads no value through its NULL pointers
    return by_types(idx_dtype, out_values ? val_dtype : OFX_DT_FLOAT, [&](auto* tp, auto* ip) -> int {
      using T = std::remove_pointer_t<decltype(tp)>;
      using I = std::remove_pointer_t<decltype(ip)>;
      return launch_rows<I, T, true>(s, k, n, (const I*)rp_a, (const I*)ci_a, (const T*)va,
                                     (const I*)rp_b, (const I*)ci_b, (const T*)vb,
                                     (const I*)row_ptr_c, (I*)out_col_idx, (T*)out_values,
                                     (char*)workspace, w);
    });
  });
}
