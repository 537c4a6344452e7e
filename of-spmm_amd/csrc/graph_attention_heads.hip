// graph_attention_heads.hip — op "graph_attention_csr_heads" on gfx950: dot-product graph
// attention over a CSR for H heads of width D,
//   attn = edge_softmax_csr_heads(sddmm_csr_heads(q, k)),  out = spmm_csr_heads(attn, v),
// with exactly the bits of that composition (contract in include/ofx_spmm.h).
//
// A row of at most `split` nonzeros (the SpMM's hub threshold, resolve_schedule(D, opts): the row
// is one sum from +0) is one work item of the main launch, owned by a group of G lanes sized from
// H*D as spmm_heads.hip sizes its group (a lane per 16 bytes of the row).  It goes through three
// phases inside the kernel:
//   1  scores:  the q row in registers, each K row read once, the per-head segmented butterfly;
//      the scores, rounded to T, are stored to attn (heads_steps.h sddmm_heads_item, the code of
//      sddmm_heads.hip with the row as its item)
//   2  softmax: the scores re-read from attn with lane <-> leaf of 8 positions, normalised in
//      place (edge_softmax.h row_in_registers / row_by_wave, the code of edge_softmax_heads.hip);
//      a row longer than 8 G positions is taken over by the whole wave, as there
//   3  aggregation: each lane loads its head's weight attn[j*H + h] itself, the V row gathered
//      with 16-byte loads (heads_steps.h spmm_heads_accumulate, the loop of spmm_heads.hip)
// Hand-off: other lanes of the same wave read what a lane stored to attn, so between two phases
// stand the plain stores, a wait for them and a workgroup-scope fence.  A wave never shares a row
// with another wave, so there is no barrier.
//
// Hub rows (more than `split` nonzeros) cannot stay with one lane group: the products-shaped graph
// of the benchmark has a row of 307,812 nonzeros and 17.7 % of its nonzeros in rows above 512, and
// one group per row took 195-246 ms there.  They go through the shared planner's
// work list (spmm_plan.h), whose chunks are the SpMM contract's: the main launch forms the scores
// of each hub chunk as an item of its own (phase 1 only), and three small launches follow on the
// same stream: the hubs' softmax (a wave per hub and head vector, in place), the chunks' partial
// sums from +0, and their addition in chunk order (the last chunk takes the remainder).  The
// planner also orders the other rows by degree (heavy rows first), as for every planned op.
//   fast path:    D % 8 == 0, D / 8 a power of two, H*D <= 2048, H a multiple of the softmax's
//                 head vector, every base and stride 16-byte aligned, K > 0
//   general path: anything else; scalar loads, a head at a time in phase 1; the same bits
// No atomics on the outputs, no allocation, no host synchronisation, no LDS, no scratch.
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>

#include "edge_softmax.h"
#include "graph_attention.h"
#include "heads_steps.h"
#include "spmm_items_dev.h"

namespace ofx {
namespace {

using namespace item;

// What a phase stored to attn is read by other lanes of the wave in the next one.
__device__ __forceinline__ void phase_handoff() {
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
}

// The launch's outputs filled with the canonical quiet NaN when the work list is not valid
// (spmm_items_dev.h plan_failed): out's rows and attn's nonzeros of the row range.
template <typename T, typename I>
__device__ __forceinline__ bool poison_outputs(const unsigned long long* __restrict__ counters,
                                               int64_t block_base, unsigned* err,
                                               const I* __restrict__ rp, int64_t row_begin,
                                               int64_t nrows, int64_t n, int64_t heads,
                                               T* __restrict__ out, int64_t ldo, T* attn) {
  if (!poison_rows(counters, block_base, err, out, ldo, (I*)nullptr, (int64_t)0, nrows, n))
    return false;
  const int64_t e0 = (int64_t)rp[row_begin] * heads, e1 = (int64_t)rp[row_begin + nrows] * heads;
  const T p = poison_value<T>();
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t e = e0 + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < e1; e += stride)
    attn[e] = p;
  return true;
}

// The main launch.  A work item is a whole row of at most `split` nonzeros, which goes through
// the three phases here, or a hub chunk (it.slot >= 0), whose scores alone are formed here: the
// hub's softmax and aggregation follow in launches of their own (below).
template <typename T, typename I, int VEC, int G, int L, bool FAST>
__global__ void __launch_bounds__(kBlock)
    graph_attention_heads_kernel(const I* __restrict__ rp, const I* __restrict__ col,
                                 const T* __restrict__ q, int64_t ldq, const T* __restrict__ kmat,
                                 int64_t ldk, const T* __restrict__ vmat, int64_t ldv, int64_t kb,
                                 T* __restrict__ out, int64_t ldo, T* attn, int64_t row_begin,
                                 int64_t nrows, int64_t n, int64_t heads, int64_t d, int lh,
                                 int64_t chunk, const unsigned long long* __restrict__ counters,
                                 const int64_t* __restrict__ items,
                                 const int64_t* __restrict__ order, int64_t block_base,
                                 unsigned* err) {
#pragma clang fp contract(off)
  using A = typename Num<T>::acc;
  constexpr int GPW = 64 / G;
  constexpr int U1 = L >= 4 ? 2 : 4;  // nonzeros in flight: the scores, the aggregation
  constexpr int U3 = 8;
  constexpr int SV = FAST ? esmh::packed_heads<T>() : 1;  // heads a lane holds in the softmax
  constexpr int NV = FAST ? 1 : VEC;
  if (poison_outputs(counters, block_base, err, rp, row_begin, nrows, n, heads, out, ldo, attn))
    return;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int gl = lane & (G - 1);
  const int gbase = lane & ~(G - 1);
  const int64_t g = ((block_base + (int64_t)blockIdx.x) * (kBlock / 64) + wave) * GPW + lane / G;
  // a group without an item keeps running with an empty row: the wave's take-overs need it
  Item it;
  const bool any = work_item<I>(rp, g, row_begin, nrows, chunk, counters, items, order, &it);
  const bool has = any && it.slot < 0;  // a whole row: all three phases
  const int64_t j0 = any ? it.j0 : 0, j1 = any ? it.j1 : 0;
  const int64_t len = has ? j1 - j0 : 0;

  // ---- phase 1: the scores (of a row or of a hub chunk) ----------------------------------------
  if (j1 > j0) {
    if constexpr (FAST) {
      hsteps::sddmm_heads_item<T, I, G, L, U1, true>(col, q + it.lr * ldq, kmat, ldk, kb, attn,
                                                     heads, d, lh, 0, j0, j1, gl, gbase);
    } else {
      for (int64_t h = 0; h < heads; ++h)
        hsteps::sddmm_heads_item<T, I, G, L, U1, false>(col, q + it.lr * ldq, kmat, ldk, kb, attn,
                                                        heads, d, 0, h, j0, j1, gl, gbase);
    }
  }
  phase_handoff();

  // ---- phase 2: the softmax along the row, in place, SV heads at a time ------------------------
  const int64_t off = j0 * heads;
  if constexpr (G == 64) {
    for (int64_t h0 = 0; h0 < heads; h0 += SV)
      esmh::row_by_wave<T, SV, false>(attn, nullptr, attn, heads, off + h0, len, lane);
  } else {
    const bool fits = len <= (int64_t)G * esm::kLeaf;
    for (int64_t h0 = 0; h0 < heads; h0 += SV)
      esmh::row_in_registers<T, SV, G, false>(attn, nullptr, attn, heads, off + h0, fits ? len : 0,
                                              gl);
    // the rows that do not fit their group: the whole wave, one after another
    unsigned long long todo = __ballot(!fits && gl == 0);
    while (todo != 0) {
      const int src = __ffsll((long long)todo) - 1;
      todo &= todo - 1;
      const int64_t woff = __shfl(off, src, 64), wlen = __shfl(len, src, 64);
      for (int64_t h0 = 0; h0 < heads; h0 += SV)
        esmh::row_by_wave<T, SV, false>(attn, nullptr, attn, heads, woff + h0, wlen, lane);
    }
  }
  phase_handoff();

  // ---- phase 3: the aggregation (a row of at most `split` nonzeros: one sum from +0) -----------
  if (!has) return;
  for (int64_t c0 = 0; c0 < n; c0 += (int64_t)G * VEC) {
    const int64_t cb = c0 + (int64_t)gl * VEC;
    // the head of each of the lane's columns (a column >= n: head 0, its product is never stored)
    int64_t hd[NV];
#pragma unroll
    for (int e = 0; e < NV; ++e) hd[e] = cb + e < n ? (cb + e) / d : 0;
    A acc[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) acc[e] = A(0);
    hsteps::spmm_heads_accumulate<T, I, VEC, G, U3, FAST>(col, attn, vmat, ldv, kb, n, heads, cb,
                                                          hd, j0, j1, gl, gbase, acc);
    T o[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) o[e] = Num<T>::store(acc[e]);
    store_cols<T, VEC, FAST>(out + it.lr * ldo, cb, n, o);
  }
}

// The hubs' softmax: a wave per (hub, SV heads), in place on the scores the main launch stored.
template <typename T, typename I, int SV>
__global__ void __launch_bounds__(kBlock)
    gat_hub_softmax_kernel(const I* __restrict__ rp, T* attn, int64_t row_begin, int64_t nrows,
                           int64_t heads, const unsigned long long* __restrict__ counters,
                           const int64_t* __restrict__ hubs, int64_t max_hubs) {
#pragma clang fp contract(off)
  if (!plan::plan_valid(counters)) return;  // the main launch has poisoned the outputs
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t hgs = heads / SV;
  const int64_t w = (int64_t)blockIdx.x * (kBlock / 64) + wave;
  const int64_t nhubs = (int64_t)counters[1] < max_hubs ? (int64_t)counters[1] : max_hubs;
  for (int64_t i = w; i < nhubs * hgs; i += (int64_t)gridDim.x * (kBlock / 64)) {
    const int64_t hub = i / hgs, hg = i - hub * hgs;
    const int64_t lr = hubs[3 * hub];
    if ((uint64_t)lr >= (uint64_t)nrows) continue;  // never from a valid plan
    const int64_t j0 = (int64_t)rp[row_begin + lr], j1 = (int64_t)rp[row_begin + lr + 1];
    esmh::row_by_wave<T, SV, false>(attn, nullptr, attn, heads, j0 * heads + hg * SV, j1 - j0, lane);
  }
}

// The hubs' aggregation: a lane group per hub chunk, summed from +0 into the chunk's partial
// (spmm_heads.hip's chunk items); hub_sum_kernel adds the partials in chunk order.
template <typename T, typename I, int VEC, int G, bool FAST>
__global__ void __launch_bounds__(kBlock)
    gat_hub_chunks_kernel(const I* __restrict__ rp, const I* __restrict__ col, const T* attn,
                          const T* __restrict__ vmat, int64_t ldv, int64_t kb, int64_t row_begin,
                          int64_t nrows, int64_t n, int64_t heads, int64_t d, int64_t chunk,
                          const unsigned long long* __restrict__ counters,
                          const int64_t* __restrict__ items, const int64_t* __restrict__ order,
                          typename Num<T>::acc* __restrict__ part, int64_t block_base) {
#pragma clang fp contract(off)
  using A = typename Num<T>::acc;
  constexpr int GPW = 64 / G;
  constexpr int U3 = 8;
  constexpr int NV = FAST ? 1 : VEC;
  if (!plan::plan_valid(counters)) return;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int gl = lane & (G - 1);
  const int gbase = lane & ~(G - 1);
  const int64_t g = ((block_base + (int64_t)blockIdx.x) * (kBlock / 64) + wave) * GPW + lane / G;
  if (g >= (int64_t)counters[0]) return;  // the chunk items come first in the work list
  Item it;
  if (!work_item<I>(rp, g, row_begin, nrows, chunk, counters, items, order, &it)) return;
  for (int64_t c0 = 0; c0 < n; c0 += (int64_t)G * VEC) {
    const int64_t cb = c0 + (int64_t)gl * VEC;
    int64_t hd[NV];
#pragma unroll
    for (int e = 0; e < NV; ++e) hd[e] = cb + e < n ? (cb + e) / d : 0;
    A acc[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) acc[e] = A(0);
    hsteps::spmm_heads_accumulate<T, I, VEC, G, U3, FAST>(col, attn, vmat, ldv, kb, n, heads, cb,
                                                          hd, it.j0, it.j1, gl, gbase, acc);
#pragma unroll
    for (int e = 0; e < VEC; ++e)
      if (cb + e < n) part[it.slot * n + cb + e] = acc[e];
  }
}

struct GatArgs {
  hipStream_t s;
  const void *rp, *col, *q, *k, *v;
  void *out, *attn;
  int64_t ldq, ldk, ldv, ldo, kk, m, row_begin, nrows, heads, d, nnz;
  void* ws;
  size_t ws_bytes;
  const ofx_spmm_options* opts;
};

template <typename T, typename I, int G, int L, bool FAST>
int gat_cfg(const GatArgs& a) {
  using A = typename Num<T>::acc;
  constexpr int VEC = 16 / sizeof(T);
  constexpr int SV = FAST ? esmh::packed_heads<T>() : 1;
  constexpr int64_t GPB = (kBlock / 64) * (64 / G);
  const int64_t n = a.heads * a.d;
  const int lh = FAST ? (int)(a.d / hsteps::kLeaf) : 0;
  const I* rp = static_cast<const I*>(a.rp);
  const I* col = static_cast<const I*>(a.col);
  T* attn = static_cast<T*>(a.attn);
  Planned p;
  int rc = prepare_plan<I>("graph_attention_csr_heads", a.s, rp, a.row_begin, a.nrows, a.nnz,
                           launch_nnz(a.m, a.nrows, a.nnz, a.opts), n, sizeof(A),
                           resolve_schedule(a.d, a.opts), false, a.ws, a.ws_bytes, &p);
  if (rc) return rc;
  A* part = static_cast<A*>(p.wl.part);
  rc = launch_cut_grid(p.work, GPB, [&](dim3 grid, int64_t b0) {
    hipLaunchKernelGGL((graph_attention_heads_kernel<T, I, VEC, G, L, FAST>), grid, dim3(kBlock), 0,
                       a.s, rp, col, static_cast<const T*>(a.q), a.ldq, static_cast<const T*>(a.k),
                       a.ldk, static_cast<const T*>(a.v), a.ldv, a.kk, static_cast<T*>(a.out),
                       a.ldo, attn, a.row_begin, a.nrows, n, a.heads, a.d, lh, p.chunk,
                       p.wl.counters, p.wl.items, p.wl.order, b0, p.err);
  });
  if (rc || !p.has_plan || p.w.max_hubs == 0) return rc;
  // the hubs: their softmax, their chunks' partials, their rows of out
  const int64_t waves = std::min<int64_t>(p.w.max_hubs * (a.heads / SV), (int64_t)8192 * 4);
  hipLaunchKernelGGL((gat_hub_softmax_kernel<T, I, SV>),
                     dim3((unsigned)((waves + kBlock / 64 - 1) / (kBlock / 64))), dim3(kBlock), 0,
                     a.s, rp, attn, a.row_begin, a.nrows, a.heads, p.wl.counters, p.wl.hubs,
                     p.w.max_hubs);
  OFX_HIP_CHECK(hipGetLastError());
  rc = launch_cut_grid(p.w.max_chunks, GPB, [&](dim3 grid, int64_t b0) {
    hipLaunchKernelGGL((gat_hub_chunks_kernel<T, I, VEC, G, FAST>), grid, dim3(kBlock), 0, a.s, rp,
                       col, attn, static_cast<const T*>(a.v), a.ldv, a.kk, a.row_begin, a.nrows, n,
                       a.heads, a.d, p.chunk, p.wl.counters, p.wl.items, p.wl.order, part, b0);
  });
  if (rc) return rc;
  return launch_hub_sum(a.s, p, static_cast<T*>(a.out), a.ldo, a.nrows, n);
}

// The lane group: a lane per 16 bytes of the H*D row, as spmm_heads.hip; at 64 lanes the leaves a
// lane holds in phase 1 grow with the width phase 1 has to cover (H*D, on the general path D).
template <typename T, typename I, bool FAST>
int gat_width(const GatArgs& a) {
  constexpr int VEC = 16 / sizeof(T);
  const int64_t n = a.heads * a.d;
  const int64_t lanes = (n + VEC - 1) / VEC;
  if (lanes <= 1) return gat_cfg<T, I, 1, 1, FAST>(a);
  if (lanes <= 4) return gat_cfg<T, I, 4, 1, FAST>(a);
  if (lanes <= 16) return gat_cfg<T, I, 16, 1, FAST>(a);
  if (lanes <= 32) return gat_cfg<T, I, 32, 1, FAST>(a);
  const int64_t w = FAST ? n : a.d;
  if (w <= 64 * hsteps::kLeaf) return gat_cfg<T, I, 64, 1, FAST>(a);
  if constexpr (FAST) {
    if (w <= 128 * hsteps::kLeaf) return gat_cfg<T, I, 64, 2, true>(a);
  }
  return gat_cfg<T, I, 64, 4, FAST>(a);
}

template <typename T, typename I>
int gat_typed(const GatArgs& a) {
  constexpr int SV = esmh::packed_heads<T>();
  const bool fast = hsteps::fast_score_shape(a.heads, a.d, a.kk) && a.heads % SV == 0 &&
                    rows_aligned(a.q, a.ldq, sizeof(T), hsteps::kLeaf) &&
                    rows_aligned(a.k, a.ldk, sizeof(T), hsteps::kLeaf) &&
                    rows_aligned(a.v, a.ldv, sizeof(T), hsteps::kLeaf) &&
                    rows_aligned(a.out, a.ldo, sizeof(T), hsteps::kLeaf) &&
                    (uintptr_t)a.attn % (SV * sizeof(T)) == 0;
  return fast ? gat_width<T, I, true>(a) : gat_width<T, I, false>(a);
}

}  // namespace
}  // namespace ofx

using namespace ofx;

extern "C" int ofx_graph_attention_csr_heads_workspace_size(int idx_dtype, int val_dtype, int64_t m,
                                                            int64_t k, int64_t heads, int64_t d,
                                                            int64_t nnz,
                                                            const ofx_spmm_options* opts,
                                                            size_t* bytes) {
  return ::ofx::guarded(__func__, [&]() -> int {
    OFX_REQUIRE(bytes != nullptr, OFX_EINVAL, "graph_attention_csr_heads_workspace_size: NULL bytes");
    OFX_READ_OPTIONS(opts, "graph_attention_csr_heads_workspace_size");
    gat::Shape sh;
    if (const int rc = gat::check_graph_attention_args(
            "graph_attention_csr_heads_workspace_size", idx_dtype, val_dtype, m, k, heads, d, nnz,
            nullptr, nullptr, nullptr, heads * d, nullptr, heads * d, nullptr, heads * d, nullptr,
            heads * d, nullptr, 0, 0, opts, &sh))
      return rc;
    sh.n = heads * d;
    *bytes = sh.n == 0 ? 0
                       : plan::ws_layout(m, nnz, sh.n, val_dtype == OFX_DT_DOUBLE ? 8 : 4,
                                         resolve_schedule(d, opts)).total;
    return OFX_OK;
  });
}

extern "C" int ofx_graph_attention_csr_heads(void* stream, int idx_dtype, int val_dtype, int64_t m,
                                             int64_t k, int64_t heads, int64_t d, int64_t nnz,
                                             const void* row_ptr, const void* col_idx,
                                             const void* q, int64_t ldq, const void* kmat,
                                             int64_t ldk, const void* v, int64_t ldv, void* out,
                                             int64_t ldo, void* attn, int64_t row_begin,
                                             int64_t row_end, void* workspace,
                                             size_t workspace_bytes,
                                             const ofx_spmm_options* opts) {
  return ::ofx::guarded(__func__, [&]() -> int {
    OFX_DEVICE_ENTRY("graph_attention_csr_heads", opts, workspace, workspace_bytes);
    gat::Shape sh;
    if (const int rc = gat::check_graph_attention_args(
            "graph_attention_csr_heads", idx_dtype, val_dtype, m, k, heads, d, nnz, row_ptr,
            col_idx, q, ldq, kmat, ldk, v, ldv, out, ldo, attn, row_begin, row_end, opts, &sh))
      return rc;
    if (sh.nothing) return OFX_OK;
    const size_t need = plan::ws_layout(sh.nrows, nnz, sh.n, val_dtype == OFX_DT_DOUBLE ? 8 : 4,
                                        resolve_schedule(d, opts)).total;
    if (const int rc =
            check_workspace("graph_attention_csr_heads", workspace, workspace_bytes, need))
      return rc;
    const GatArgs a{static_cast<hipStream_t>(stream), row_ptr, col_idx, q, kmat, v, out, attn, ldq,
                    ldk, ldv, ldo, k, m, row_begin, sh.nrows, heads, d, nnz, workspace,
                    workspace_bytes, opts};
    return by_types(idx_dtype, val_dtype, [&](auto* tp, auto* ip) -> int {
      return gat_typed<std::remove_pointer_t<decltype(tp)>, std::remove_pointer_t<decltype(ip)>>(a);
    });
  });
}
