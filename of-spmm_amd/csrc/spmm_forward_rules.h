#ifndef OFX_SPMM_FORWARD_RULES_H_
#define OFX_SPMM_FORWARD_RULES_H_
// spmm_forward_rules.h — the host side of the SpMM forward: the launchers of the kernels in
// spmm_csr_impl.h, the configuration families (Cfg with a family's fixed parameters named once)
// and the ordered rules by which launch_typed picks a configuration for a launch whose form
// spmm_launch.h has decided (DESIGN.md §3 "Forms").  Included by the per-type instantiation units
// (spmm_inst_*.hip) and the tuning table (spmm_csr_tuned.hip) only.
#pragma clang fp contract(off)

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <type_traits>

#include "spmm_csr_impl.h"

namespace ofx {
namespace {

template <typename T, int VEC>
int launch_reduce_vec(hipStream_t s, int64_t max_hubs, int64_t n,
                      const unsigned long long* counters, const int64_t* hubs,
                      const typename Num<T>::acc* part, T* C, int64_t ldc, const T* bias, int act) {
  const int64_t lanes = (n + VEC - 1) / VEC;
  int l = 4;
  while (l < 64 && l < lanes) l *= 2;
  const int64_t per_block = kBlock / l;
  int64_t grid = (max_hubs + per_block - 1) / per_block;
  if (grid > kMaxReduceBlocks) grid = kMaxReduceBlocks;
#define OFX_REDUCE(LL)                                                                        \
  hipLaunchKernelGGL((spmm_reduce_kernel<T, VEC, LL>), dim3((unsigned)grid), dim3(kBlock), 0, s, \
                     counters, hubs, part, C, ldc, n, bias, act)
  switch (l) {
    case 4: OFX_REDUCE(4); break;
    case 8: OFX_REDUCE(8); break;
    case 16: OFX_REDUCE(16); break;
    case 32: OFX_REDUCE(32); break;
    default: OFX_REDUCE(64); break;
  }
#undef OFX_REDUCE
  OFX_HIP_CHECK(hipGetLastError());
  return OFX_OK;
}

// 16-B partial loads when every partial row starts 16-B aligned (the workspace base is 256-B
// aligned and rows are n accumulators apart), else one accumulator per lane.
template <typename T>
int launch_reduce(hipStream_t s, int64_t max_hubs, int64_t n, const unsigned long long* counters,
                  const int64_t* hubs, const typename Num<T>::acc* part, T* C, int64_t ldc,
                  const T* bias, int act) {
  using A = typename Num<T>::acc;
  constexpr int kVec = 16 / (int)sizeof(A);
  if ((n * (int64_t)sizeof(A)) % 16 == 0)
    return launch_reduce_vec<T, kVec>(s, max_hubs, n, counters, hubs, part, C, ldc, bias, act);
  return launch_reduce_vec<T, 1>(s, max_hubs, n, counters, hubs, part, C, ldc, bias, act);
}

int pick_vec(int elem_bytes, const Launch& L, int forced_vec, int cap = 16) {
  const int maxvec = std::min(16 / elem_bytes, cap);
  for (int v = maxvec; v >= 1; v /= 2) {
    if (forced_vec && v != forced_vec) continue;
    const size_t vb = (size_t)v * elem_bytes;
    if (L.n % v == 0 && L.ldb % v == 0 && L.ldc % v == 0 &&
        ((uintptr_t)L.b % vb) == 0 && ((uintptr_t)L.c % vb) == 0)
      return v;
  }
  return 0;
}

int pick_lpr(int64_t n, int vec) {
  const int64_t lanes = (n + vec - 1) / vec;
  int l = 4;
  while (l < 64 && l < lanes) l *= 2;
  return l;
}

// ofx_spmm_csr_describe: the configuration a launch takes (kind = "main" for the planned forms'
// spmm_main_kernel, "small" for spmm_small_kernel), written instead of launching.  The form names
// follow DESIGN.md §3: small, mid (block items), narrow (wave items of HL lanes), prefetch (PF
// without block items), bandwidth (the rest).
template <typename T, typename I, typename K>
int describe_cfg(const Launch& L, const char* kind) {
  const char* form = std::strcmp(kind, "small") == 0 ? "small"
                     : K::BI                         ? "mid"
                     : (K::WH && K::HL > 0)          ? "narrow"
                     : K::PF                         ? "prefetch"
                                                     : "bandwidth";
  // the workspace this launch lays out (<= ofx_spmm_csr_workspace_size over the matrix's m)
  const size_t ws = std::strcmp(kind, "small") == 0
                        ? 0
                        : ws_layout(L.nrows, L.nnz, L.n, sizeof(typename Num<T>::acc), L.sched).total;
  std::snprintf(L.describe, L.describe_bytes,
                "form=%s kernel=%s VEC=%d LPR=%d U=%d WPB=%d NT=%d PF=%d WH=%d BI=%d BUF=%d SH=%d "
                "HL=%d HU=%d HV=%d XL=%d LR=%d elem=%d idx=%d ws=%zu",
                form, kind, K::VEC, K::LPR, K::U, K::WPB, (int)K::NT, (int)K::PF, (int)K::WH,
                (int)K::BI, (int)K::BUF, (int)K::SH, K::HL, K::HU, K::HV, (int)K::XL, (int)K::LR,
                (int)sizeof(T),
                (int)sizeof(I), ws);
  return OFX_OK;
}

#ifdef OFX_DEBUG_BOUNDS
// OFX_DEBUG_BOUNDS builds: the launch's allocations (dbg_bounds.h), published on its stream before
// its kernels, and its configuration as the tag recorded with a violation:
// VEC | LPR << 8 | U << 16 | flags << 24 (NT PF BNT WH BI BUF SH LR) | HL << 32 | HU << 40 |
// kind << 48
template <typename T, typename I, typename K>
int debug_publish(const Launch& L, unsigned long long kind) {
  dbg::HostBounds hb;
  const int64_t si = (int64_t)sizeof(I), st = (int64_t)sizeof(T);
  hb.add(L.rp, (uint64_t)((L.row_begin + L.nrows + 1) * si));
  hb.add(L.col, (uint64_t)(L.nnz * si));
  hb.add(L.val, (uint64_t)(L.nnz * st));
  hb.add(L.vperm, (uint64_t)(L.nnz * si));
  if (L.b_rows > 0) hb.add(L.b, (uint64_t)(((L.b_rows - 1) * L.ldb + L.n) * st));
  hb.add(L.c, (uint64_t)(((L.nrows - 1) * L.ldc + L.n) * st));
  hb.add(L.ws, L.ws_bytes);
  hb.add(L.bias, (uint64_t)(L.n * st));
  void* zero = nullptr;
  OFX_HIP_CHECK(hipGetSymbolAddress(&zero, HIP_SYMBOL(g_zero_row)));
  hb.add(zero, kZeroRowBytes);
  const unsigned long long flags = (unsigned long long)K::NT | (unsigned long long)K::PF << 1 |
                                   (unsigned long long)K::BNT << 2 | (unsigned long long)K::WH << 3 |
                                   (unsigned long long)K::BI << 4 | (unsigned long long)K::BUF << 5 |
                                   (unsigned long long)K::SH << 6 | (unsigned long long)K::LR << 7;
  const unsigned long long tag = (unsigned long long)K::VEC | (unsigned long long)K::LPR << 8 |
                                 (unsigned long long)K::U << 16 | flags << 24 |
                                 (unsigned long long)K::HL << 32 | (unsigned long long)K::HU << 40 |
                                 kind << 48;
  OFX_REQUIRE(hb.publish(L.stream, tag) == 0, OFX_EDEVICE, "spmm_csr: debug bounds not published");
  return OFX_OK;
}
#endif

template <typename T, typename I, typename K>
int launch_cfg(const Launch& L) {
  if (L.describe != nullptr) return describe_cfg<T, I, K>(L, "main");
  using A = typename Num<T>::acc;
  constexpr int GPW = 64 / K::LPR;
  constexpr int64_t GPB = (int64_t)K::WPB * GPW;  // lane-groups per block
  const I* rp = static_cast<const I*>(L.rp);
  const I* col = static_cast<const I*>(L.col);
  const T* val = static_cast<const T*>(L.val);
  const T* B = static_cast<const T*>(L.b);
  T* C = static_cast<T*>(L.c);
  const WsLayout w = ws_layout(L.nrows, L.nnz, L.n, sizeof(A), L.sched);
  const bool plan = w.total > 0;
#ifdef OFX_DEBUG_BOUNDS
  if (const int rc = debug_publish<T, I, K>(L, 1)) return rc;
#endif
  WorkList wl{};
  if (plan) {
    OFX_REQUIRE(L.ws != nullptr && L.ws_bytes >= w.total, OFX_EWORKSPACE,
                "spmm_csr: workspace of %zu bytes is smaller than the %zu bytes required",
                L.ws_bytes, w.total);
    if (L.sched.planned) {
      plan::worklist_of(w, static_cast<char*>(L.ws), &wl);
    } else {
      const int rc = launch_plan<I>(L.stream, rp, L.row_begin, L.nrows, L.nnz_est, L.sched, w,
                                    static_cast<char*>(L.ws), &wl);
      if (rc) return rc;
    }
  }
  unsigned long long* counters = wl.counters;
  int64_t *hub = wl.hubs, *items = wl.items, *order = wl.order;
  A* part = reinterpret_cast<A*>(wl.part);
  // Work items: hub chunks, heavy rows, then every row by index (surplus groups exit at once).
  // The WH / BI forms put one wave / block per hub chunk and heavy row first (upper bound: every
  // chunk and every row longer than the heavy threshold), then the groups of the rows.
  const int64_t heavy = L.sched.heavy == 0 ? auto_heavy(L.nrows, L.nnz_est) : L.sched.heavy;
  const int64_t heavy_bound =
      heavy == INT64_MAX ? 0 : std::min<int64_t>(L.nrows, L.nnz / (heavy + 1) + 1);
  const int64_t bi_items = w.max_chunks + heavy_bound;
  // wave items (one wave each) and block items (one block each) are bounded alike: hub chunks
  // plus the rows above the heavy threshold.  The wave items loop (a wave strides over them), so
  // their blocks are capped at kWaveItemBlocks; the light rows then need one group per row.
  constexpr int64_t kWaveItemBlocks = 2048;
  const bool wh = K::WH && K::LPR < 64 && plan;
  const int64_t wave_blocks = wh ? std::min<int64_t>((bi_items + K::WPB - 1) / K::WPB, kWaveItemBlocks)
                              : (K::BI && plan) ? bi_items
                                                : 0;
  const int64_t work = L.nrows + (plan && !wh && !K::BI ? bi_items : 0);
  const int64_t grid = wave_blocks + (work + GPB - 1) / GPB;
  // A launch holds fewer than 2^32 threads (papers-scale: 111M rows + items at 8 groups per block
  // would not): the grid goes out in pieces of kLaunchBlocks, each told its first block.
  constexpr int64_t kLaunchBlocks = ((int64_t)1 << 31) / (64 * K::WPB);
  for (int64_t b0 = 0; b0 < grid; b0 += kLaunchBlocks) {
    const int64_t nb = std::min(kLaunchBlocks, grid - b0);
    hipLaunchKernelGGL((spmm_main_kernel<T, I, K>), dim3((unsigned)nb), dim3(64 * K::WPB), 0,
                       L.stream, rp, col, val, static_cast<const I*>(L.vperm), B, L.ldb, L.b_rows,
                       C, L.ldc, L.row_begin, L.nrows, L.n, plan ? L.sched.split : INT64_MAX,
                       plan ? L.sched.chunk : INT64_MAX, heavy, counters, items, order, part,
                       static_cast<const T*>(L.bias), L.act, wave_blocks, b0, wl.arrive,
                       plan ? device_error_words() : nullptr);
    OFX_HIP_CHECK(hipGetLastError());
  }
  if (plan && w.max_hubs > 0 && !K::LR)  // LR: the main kernel added the hubs (hub_tail)
    return launch_reduce<T>(L.stream, w.max_hubs, L.n, counters, hub, part, C, L.ldc,
                            static_cast<const T*>(L.bias), L.act);
  return OFX_OK;
}


template <typename T, typename I, typename K>
int launch_small(const Launch& L) {
  if (L.describe != nullptr) return describe_cfg<T, I, K>(L, "small");
  using SF = SmallForm<T, I, K>;
  // options.heavy_threshold > 0 overrides the light/whole-block cut (tuning; no numeric effect)
  const int64_t light =
      (L.sched.heavy > 0 && L.sched.heavy != INT64_MAX) ? L.sched.heavy : (int64_t)kSmallLight * K::U;
  const int64_t grid = (L.nrows + SF::RPB - 1) / SF::RPB;
#ifdef OFX_DEBUG_BOUNDS
  if (const int rc = debug_publish<T, I, K>(L, 2)) return rc;
#endif
  OFX_REQUIRE(grid < (int64_t)UINT32_MAX, OFX_EINVAL, "spmm_csr: too many rows (%lld)",
              (long long)L.nrows);
  hipLaunchKernelGGL((spmm_small_kernel<T, I, K>), dim3((unsigned)grid), dim3(64 * K::WPB), 0,
                     L.stream, static_cast<const I*>(L.rp), static_cast<const I*>(L.col),
                     static_cast<const T*>(L.val), static_cast<const I*>(L.vperm),
                     static_cast<const T*>(L.b), L.ldb, L.b_rows, static_cast<T*>(L.c), L.ldc,
                     L.row_begin,
                     L.nrows, L.n, L.sched.split, L.sched.chunk, light,
                     static_cast<const T*>(L.bias), L.act);
  OFX_HIP_CHECK(hipGetLastError());
  return OFX_OK;
}

// A small-form configuration: the small kernel.  (launch_form sends no other launch here; the
// planned branch keeps the main kernels of these configurations in the library.)
template <typename T, typename I, typename K>
int launch_small_or_planned(const Launch& L, Form form) {
  if (form == Form::Small) return launch_small<T, I, K>(L);
  return launch_cfg<T, I, K>(L);
}

// B far larger than the Infinity Cache (> 1 GiB): the col/val/C streams are loaded and stored
// non-temporally so they do not evict the hot (hub) B rows that still hit on-die.  Measured
// (scripts/ab.py, bit-identical): papers-scale -1.8%, products -0.3%; with B at cache size
// (1M power-law, 256 MB) the same hint costs +8%, hence the threshold.
constexpr int64_t kNtBytes = int64_t(1) << 30;

// B's byte offsets fit the buffer descriptor's 32 bits (BRows): row k (the zero row) included.
template <typename T>
bool buffer_rows_ok(const Launch& L) {
  return (unsigned __int128)(L.b_rows + 1) * (unsigned __int128)L.ldb * sizeof(T) <
         ((unsigned __int128)1 << 32);
}

// b and c at element alignment (a view may start at any element).
template <typename T>
bool element_aligned(const Launch& L) {
  return ((uintptr_t)L.b % sizeof(T)) == 0 && ((uintptr_t)L.c % sizeof(T)) == 0;
}

// ---- configuration families --------------------------------------------------------------------
// Cfg<VEC, LPR, U, WPB, NT, PF, BNT, WH, BI, BUF, HL, HU, SH, LR, HV, XL> (spmm_csr_impl.h) with
// the parameters a family fixes written once, by name; an alias takes the ones that vary within
// its family.  The kernels' names are Cfg's, so an alias and the spelled-out Cfg are one kernel.

// f(std::integral_constant<int, LPR>) for a run-time lane count: a family's instantiation per
// lanes-per-row (4 .. 64; a forced layout can ask for any other).
template <typename F>
int with_lanes(int lpr, F&& f) {
  switch (lpr) {
    case 4: return f(std::integral_constant<int, 4>{});
    case 8: return f(std::integral_constant<int, 8>{});
    case 16: return f(std::integral_constant<int, 16>{});
    case 32: return f(std::integral_constant<int, 32>{});
    case 64: return f(std::integral_constant<int, 64>{});
    default: return fail(OFX_EINVAL, "spmm_csr: unsupported lanes-per-row %d", lpr);
  }
}

// B-row loads in flight per lane of the small-launch configurations: 32, 16 for 8-16 B lanes.
template <typename T, int VEC>
constexpr int kSmallLaunchLoads = VEC * sizeof(T) <= 4 ? 32 : 16;

// Small problems (<= kSmallRows rows: too few lane-groups to be bandwidth-bound) run as long as
// their longest non-split row, a chain of len / U dependent B-row load rounds; these launches keep
// 32 (16 for 8-16 B lanes) loads in flight per lane instead of 8.  A Cora-shaped layer (max row
// 253 nonzeros, N=16) took 25 us with U=8.  Same bits: U only changes how many loads are issued
// ahead of the in-order adds.  Below kSmallFormElems products the launch is the small form.
// 64 lanes (one row per wave) run without the prefetch and the wave items.
template <typename T, int VEC, int LPR>
using SmallCfg = Cfg<VEC, LPR, kSmallLaunchLoads<T, VEC>, /*WPB*/ 4, /*NT*/ false,
                     /*PF*/ (LPR < 64), /*BNT*/ false, /*WH*/ (LPR < 64)>;

// The prefetching form (Form::Prefetch): U = 32 / 16 loads in flight per lane, the next batch's
// (col, val) prefetched; WH: hub chunks and heavy rows take a whole wave (wave items).  Tuning
// variants 30004 (WH) / 30005 force it at any size.
// 64 lanes as in the small family; hubs added in the kernel (LR).
template <typename T, int VEC, int LPR, bool WH>
using PrefetchCfg = Cfg<VEC, LPR, kSmallLaunchLoads<T, VEC>, /*WPB*/ 4, /*NT*/ false,
                        /*PF*/ (LPR < 64), /*BNT*/ false, /*WH*/ (WH && LPR < 64), /*BI*/ false,
                        /*BUF*/ true, /*HL*/ 0, /*HU*/ 16, /*SH*/ false, /*LR*/ kLR>;

// Mid form (Form::Mid): block items first, then one lane-group per light row.  SR: the light
// rows run the small-launch configuration (U = 32 / 16 loads in flight, next batch prefetched)
// instead of the big-launch one (U = 8, 16 for one-element fp32 lanes).
// The prefetch goes with SR at every lane count, 64 included.
template <typename T, int VEC, int LPR, bool SR>
using MidCfg = Cfg<VEC, LPR,
                   SR ? kSmallLaunchLoads<T, VEC> : (VEC == 1 && sizeof(T) == 4 ? 16 : 8),
                   /*WPB*/ 4, /*NT*/ false, /*PF*/ SR, /*BNT*/ false, /*WH*/ false, /*BI*/ true,
                   /*BUF*/ true, /*HL*/ 0, /*HU*/ 16, /*SH*/ false, /*LR*/ kLR>;

// The bandwidth configuration: U = 8 loads in flight, the col / val / C streams non-temporal (NT)
// past kNtBytes of B.  Three families over the same parameters: buffer loads, global loads (B of
// 4 GiB or more, papers-scale: BUF = false) and the shifted last window (SH, launch_shift).
template <int VEC, int LPR, int U, bool NT>
using BandwidthCfg = Cfg<VEC, LPR, U, /*WPB*/ 4, NT>;
template <int VEC, int LPR, int U, bool NT>
using GlobalCfg = Cfg<VEC, LPR, U, /*WPB*/ 4, NT, /*PF*/ false, /*BNT*/ false, /*WH*/ false,
                      /*BI*/ false, /*BUF*/ false>;
template <int VEC, int LPR, int U, bool NT>
using ShiftCfg = Cfg<VEC, LPR, U, /*WPB*/ 4, NT, /*PF*/ false, /*BNT*/ false, /*WH*/ false,
                     /*BI*/ false, /*BUF*/ true, /*HL*/ 0, /*HU*/ 16, /*SH*/ true>;

// A bandwidth family's configuration for `lpr` lanes.  NT kernels exist at 32 and 64 lanes only:
// narrower rows keep the plain streams whatever `nt` says.
template <typename T, typename I, template <int, int, int, bool> class Family, int VEC>
int launch_bandwidth(const Launch& L, int lpr, bool nt) {
  return with_lanes(lpr, [&](auto lanes) {
    constexpr int LPR = decltype(lanes)::value;
    // fp32 rows of <= 64 B (one element per lane): 16 loads in flight instead of 8, -1.2% on
    // products-shaped N = 16 (tuning variant 10021, profiles/r02_ab_n16_bnt.log), same bits.
    // (No else: the U = 8 kernel of this layout stays in the library, though no launch takes it.)
    if constexpr (LPR == 16 && VEC == 1 && sizeof(T) == 4)
      return launch_cfg<T, I, Family<1, 16, 16, false>>(L);
    if constexpr (LPR >= 32) {
      if (nt) return launch_cfg<T, I, Family<VEC, LPR, 8, true>>(L);
    }
    return launch_cfg<T, I, Family<VEC, LPR, 8, false>>(L);
  });
}

// The generic path: the form's family at the chosen vector width and lane count.
template <typename T, typename I, int VEC>
int launch_vec(const Launch& L, Form form, const FormExtras& x, int lpr, bool nt) {
  if (!buffer_rows_ok<T>(L)) {
    const int v = L.sched.variant;
    OFX_REQUIRE(v == 0 || (v > 0 && form == Form::Bandwidth), OFX_EINVAL,
                "spmm_csr: variant %d needs B under 4 GiB (k=%lld, ldb=%lld)", v,
                (long long)L.b_rows, (long long)L.ldb);
    return launch_bandwidth<T, I, GlobalCfg, VEC>(L, lpr, nt);
  }
  if (form == Form::Bandwidth)
    return x.global_loads ? launch_bandwidth<T, I, GlobalCfg, VEC>(L, lpr, nt)
                          : launch_bandwidth<T, I, BandwidthCfg, VEC>(L, lpr, nt);
  return with_lanes(lpr, [&](auto lanes) {
    constexpr int LPR = decltype(lanes)::value;
    switch (form) {
      case Form::Small: return launch_small_or_planned<T, I, SmallCfg<T, VEC, LPR>>(L, form);
      case Form::Mid:
        return x.small_rows ? launch_cfg<T, I, MidCfg<T, VEC, LPR, true>>(L)
                            : launch_cfg<T, I, MidCfg<T, VEC, LPR, false>>(L);
      default:  // Form::Prefetch
        return x.wave_items ? launch_cfg<T, I, PrefetchCfg<T, VEC, LPR, true>>(L)
                            : launch_cfg<T, I, PrefetchCfg<T, VEC, LPR, false>>(L);
    }
  });
}

// fp32 rows whose width is not a multiple of 4 above N = 64 in the bandwidth configuration:
// 16-B lanes with the last window shifted (Cfg::SH) instead of one element per lane, which needs
// several 64-lane passes there: products N = 99 / 301 10.6 / 31.2 -> 8.5 / 25.2 ms.  At 17-63
// columns one pass of single elements is as fast or faster (N = 41 / 47 / 63: 4.6 / 5.0 / 6.1 ms
// against 4.8 / 5.2 / 6.2; such rows cost whole 128-B lines either way); profiles/r03ad_sweep.jsonl.
// Round 5: 16-bit rows whose width is not a multiple of 8 above N = 64 the same way (8-element
// windows at 2-B alignment, probes/unaligned_probe.hip) instead of one element per lane over 64
// lanes: 1M power-law bf16 N = 99 / 127 / 255 1,490 / 1,556 / 3,031 -> 917 / 1,040 / 1,799 us
// (tuning entries 10122 / 10123, gpurun_out/r05h_2_py.txt; N = 128 / 256: 853 / 1,489).
// And 16-bit rows of 17-63 columns (but 32) in the bandwidth form, where the N / 16-element
// lanes left them one element per lane over 32-64 lanes: 4-element windows over 8 lanes up to 31
// columns, 8-element windows over 8 lanes above (entries 10175 / 10177, gpurun_out/r05t_1_py.txt,
// 1M power-law bf16 N = 17 / 31 / 33 / 47 / 63: 521 / 551 / 823 / 841 / 862 -> 403 / 487 / 555 /
// 609 / 674 us; N = 32 / 64 369 / 465 keep their layouts).  fp32 there stays one element per
// lane: shifted windows moved it by -6..+3% on that graph and +4% on products (round 3).
template <typename T>
bool shift_rule(const Launch& L, Form form) {
  const bool odd = L.n > 64 ? L.n % (16 / (int64_t)sizeof(T)) != 0
                            : sizeof(T) == 2 && L.n > 16 && L.n < 64 && L.n != 32;
  return form == Form::Bandwidth && odd;
}

template <typename T, typename I>
int launch_shift(const Launch& L, bool nt) {
  constexpr int V = 16 / (int)sizeof(T);
  if constexpr (sizeof(T) == 2) {  // 17-31 columns: 4-element windows over 8 lanes
    if (L.n < 32) return launch_cfg<T, I, ShiftCfg<4, 8, 8, false>>(L);
  }
  return launch_bandwidth<T, I, ShiftCfg, V>(L, pick_lpr(L.n, V), nt);
}

// The prefetching form's (mid-size graphs) odd fp32 widths above 16: 16-B lanes with the shifted
// last window, U = 16 loads in flight and the next (col, val) batch prefetched, instead of one
// element per lane (N <= 64: up to 64 lanes, one row per wave).  Hubs added in the kernel (LR), as
// in the rest of the prefetching form.
// (Round 5: rows up to 128 / 256 columns take launch_mid_width_pf; this serves the wider ones,
// and 16-bit rows in 8-element windows the same way.)
template <int VEC, int LPR>
using ShiftPrefetchCfg = Cfg<VEC, LPR, /*U*/ 16, /*WPB*/ 4, /*NT*/ false, /*PF*/ (LPR < 64),
                             /*BNT*/ false, /*WH*/ false, /*BI*/ false, /*BUF*/ true, /*HL*/ 0,
                             /*HU*/ 16, /*SH*/ true, /*LR*/ kLR>;

template <typename T>
bool shift_pf_rule(const Launch& L, Form form) {
  return form == Form::Prefetch && L.n > 16 && L.n % (16 / (int64_t)sizeof(T)) != 0;
}

template <typename T, typename I>
int launch_shift_pf(const Launch& L) {
  constexpr int V = 16 / (int)sizeof(T);
  return with_lanes(pick_lpr(L.n, V), [&](auto lanes) {
    return launch_cfg<T, I, ShiftPrefetchCfg<V, decltype(lanes)::value>>(L);
  });
}

// Wave items in HL-lane groups of HV elements, HU loads in flight (the narrow and mid-width
// entries): prefetching light rows of U = 8.
template <int VEC, int LPR, int HL, int HU, bool SH, bool LR, int HV = 1, bool XL = false>
using WaveGroupCfg = Cfg<VEC, LPR, /*U*/ 8, /*WPB*/ 4, /*NT*/ false, /*PF*/ true, /*BNT*/ false,
                         /*WH*/ true, /*BI*/ false, /*BUF*/ true, HL, HU, SH, LR, HV, XL>;


// Rows of 64 B in fp32 (N = 16) above the mid form: four lanes of float4 per light row (16 rows
// per wave, few registers, so many rows in flight: what bounds these launches) and the hub chunks
// and heavy rows as wave items in 16-lane one-element groups (HL), so a 512-nonzero chunk is not
// one 4-lane chain.  Up to kPrefetchNnz: U = 4 with 16 wave-item loads in flight per lane (arxiv-
// shaped 71 -> 46 us, 2M nonzeros 65 -> 56 us); past it 2-lane float2 groups of U = 8 with 8 (5M
// 111 -> 92 us, 1M power-law 406 -> 353 us, products 2,241 -> 2,184 us; a uniform-degree 20M graph
// 396 -> 402 us).  profiles/r03n_graph.jsonl.  Same bits: only who adds changes.
// Past kPrefetchNnz only: up to it the mid-width shape below (LDS-exchanged wave items) is faster
// since round 5, when round 4's U = 8 in-kernel-reduce shape (entry 10082) gave way to it.  fp32
// rows of N = 16 with 16-B aligned b, c and strides only.
bool narrow_rule(const Launch& L, Form form) {
  return form == Form::Bandwidth && L.n == 16 && pick_vec(4, L, 0) == 4;
}

template <typename T, typename I>
int launch_narrow(const Launch& L) {
  return launch_cfg<T, I, WaveGroupCfg<2, 8, /*HL*/ 16, /*HU*/ 8, /*SH*/ false, /*LR*/ false>>(L);
}

// Narrow rows of mid-size launches (round 4, launch_narrow_pf, removed in round 5): 16-bit rows
// of 8 or 16 columns and fp32 rows of 8 took four lanes per light row (8 B per lane) with 16-lane
// one-element wave items (entries 10050-10063, profiles/r04k_variants.jsonl); the LDS-exchanged
// wave items of launch_mid_width_pf below replaced it at every such width.

// Rows of 17-64 columns of mid-size launches (round 5): the narrow form's
// shape for every width -- shifted windows (Cfg::SH, any N; 2-B-aligned 8 / 16-B accesses are
// exact and as fast on gfx950, probes/unaligned_probe.hip) over 8 lanes, hubs added in the
// kernel -- with the wave items (hub chunks, heavy rows) in 32-lane groups, one column pass
// (the reference gather's word choice, gather_kernel_util.cu:69-104, falls to 2-B words at odd
// 16-bit widths; the shifted window keeps 8 / 16-B words at any width):
// 1-element lanes up to 32 columns, 2-element lanes up to 64 (Cfg::HV).  The wave items' column
// passes were what held these widths: the round-4 layouts ran 16-lane one-element wave items, two
// to four passes per chunk.  Tuning entries 10100 / 10110 / 10117 / 10112 (profiles/
// r05_width_sweep_midsize.jsonl), arxiv-shaped 169k x 1.17M: fp32 N = 17-32 77 -> 58 us, fp32
// 33-64 97-103 -> 79-82, bf16 17 / 24 94 / 84 -> 68 / 66, bf16 33-63 125-160 -> 81-82 and N = 64
// 94 -> 79; 60k x 1.5M fp32 N = 17 72 -> 55, bf16 N = 47 / 63 118 / -> 79.  Same bits: only who
// adds changes.
// The same shape either side (entries 10130-10142, gpurun_out/r05i_1_py.txt, arxiv-shaped):
// rows of 1-15 columns (8 and 16 keep the narrow forms when aligned) in 4-lane groups, one
// element per lane below 4 columns and shifted 4-element windows above, with 16-lane wave items
// -- fp32 N = 1 / 4 / 12 / 15 75 / 86 / 73 / 83 -> 45 / 46 / 47 / 49 us, bf16 100 / 105 / 83 / 92
// -> 47 / 48 / 50 / 50; rows of 65-128 columns in 8-element windows over 16 lanes with 4-element
// wave lanes -- fp32 N = 65 / 99 / 128 143 / 148 / 147 -> 110 / 113 / 114, bf16 N = 65 / 99 / 128
// 463 / 467 / 151 -> 111 / 112 / 109; and 16-bit rows of 129-256 columns, 8-element wave lanes
// with 8 in flight -- bf16 N = 129 / 200 / 255 / 256 656 / 166 / 857 / 164 -> 155 / 150 / 158 /
// 150.  fp32 rows above 128 columns keep their layouts (as fast: 173-210 us either way).
// Up to 64 columns the wave items exchange their products through LDS (Cfg::XL,
// accumulate_wave_xl): 8- / 16-lane groups of 2-4 elements, 32-64 nonzeros per round of B-row
// loads without the cross-lane moves that made narrow groups lose (entries 10183-10198,
// gpurun_out/r05aa_2_py.txt / r05z_2_py.txt, arxiv-shaped / 60k x 1.5M): fp32 N = 8 / 12 / 16
// 43 / 44 / 44 -> 38 / 39 / 39 us, fp32 17-32 56 -> 48, fp32 47 / 64 78 -> 73 / 72 (76 -> 70),
// bf16 17 / 24 57 -> 54 / 53, bf16 47 / 64 80 / 78 -> 71 / 65 (80 / 79 -> 77 / 74); and 16-bit
// rows of 4-16 columns, aligned 8 / 16 included (round 4's narrow shape, launch_narrow_pf, is
// gone; entries 10199-10202, gpurun_out/r05ae_1_py.txt): bf16 N = 4 / 8 / 12 / 16 44 / 46 / 47 /
// 47 -> 37 / 40 / 42 / 42 us (60k x 1.5M 45 -> 43); fp32 rows of 65-128 columns too, two
// 32-lane groups of 8 nonzeros (entry 10204, gpurun_out/r05ag_2_py.txt): N = 65 / 99 / 128 107 /
// 111 / 112 -> 101 / 106 / 107 us (60k x 1.5M 101 / 106 / 107 -> 97 / 103 / 105); 16-bit rows
// there gained nothing from it (-1..+3%) and keep the cross-lane groups.  Rows of 1-3 columns:
// 16 four-lane groups of 8 nonzeros, 128 nonzeros per round of B-row loads (entry 10207,
// gpurun_out/r05aj_2_py.txt): fp32 / bf16 N = 1-3 42-45 -> 29-31 us on both mid-size graphs.
template <int VEC, int LPR, int HL, int HU, bool SH, int HV, bool XL>
using MidWidthCfg = WaveGroupCfg<VEC, LPR, HL, HU, SH, /*LR*/ kLR, HV, XL>;

template <typename T>
bool mid_width_rule(const Launch& L, Form form) {
  return form == Form::Prefetch && L.n >= 1 && L.n <= (sizeof(T) == 2 ? 256 : 128);
}

template <typename T, typename I>
int launch_mid_width_pf(const Launch& L) {
  //                                           VEC LPR  HL  HU    SH  HV    XL
  if (L.n < 4) return launch_cfg<T, I, MidWidthCfg<1, 4, 4, 8, false, 1, true>>(L);
  if (L.n <= 16) return launch_cfg<T, I, MidWidthCfg<4, 4, 8, 8, true, 2, true>>(L);
  if (L.n <= 32) return launch_cfg<T, I, MidWidthCfg<4, 8, 8, 8, true, 4, true>>(L);
  if constexpr (sizeof(T) == 2) {
    if (L.n <= 64) return launch_cfg<T, I, MidWidthCfg<8, 8, 16, 8, true, 4, true>>(L);
    if (L.n <= 128) return launch_cfg<T, I, MidWidthCfg<8, 16, 32, 16, true, 4, false>>(L);
    return launch_cfg<T, I, MidWidthCfg<8, 32, 32, 8, true, 8, false>>(L);
  } else {
    if (L.n <= 64) return launch_cfg<T, I, MidWidthCfg<4, 16, 16, 8, true, 4, true>>(L);
    return launch_cfg<T, I, MidWidthCfg<8, 16, 32, 8, true, 4, true>>(L);
  }
}

// What every special rule above needs: the automatic variant, 2- or 4-byte elements (f64 takes
// none of them), b and c at element alignment and B within a buffer descriptor's range.
template <typename T>
bool special_rules_apply(const Launch& L) {
  return L.sched.variant == 0 && sizeof(T) <= 4 && element_aligned<T>(L) && buffer_rows_ok<T>(L);
}

}  // namespace

// The configuration of a launch, by the first rule that takes it: the tuning table, the narrow
// form, the mid-width entries, the shifted bandwidth and prefetching windows, then the generic
// path (vector width, lanes, cache hint) in the form's family.
template <typename T, typename I>
int launch_typed(const Launch& L) {
  FormExtras x;
  const Form form = launch_form(L.nrows, L.nnz_est, L.n, L.sched, &x);
  const int variant = L.sched.variant;
  if (variant >= 10000 && !x.forced) {
    OFX_REQUIRE(buffer_rows_ok<T>(L), OFX_EINVAL,
                "spmm_csr: tuning variant %d needs B under 4 GiB", variant);
    return launch_tuned<T, I>(L, variant - 10000);
  }
  const bool nt = (L.b_rows * L.ldb * (int64_t)sizeof(T)) > kNtBytes;
  if constexpr (sizeof(T) <= 4) {
    if (special_rules_apply<T>(L)) {
      if constexpr (sizeof(T) == 4) {
        if (narrow_rule(L, form)) return launch_narrow<T, I>(L);
      }
      if (mid_width_rule<T>(L, form)) return launch_mid_width_pf<T, I>(L);
      if (shift_rule<T>(L, form)) return launch_shift<T, I>(L, nt);
      if (shift_pf_rule<T>(L, form)) return launch_shift_pf<T, I>(L);
    }
  }
  // variant = VEC * 100 + LPR forces a configuration (tuning / tests); 0 = auto.
  const int forced_vec = (variant > 0 && !x.forced) ? variant / 100 : 0;
  const int forced_lpr = (variant > 0 && !x.forced) ? variant % 100 : 0;
  // fp32 rows of <= 64 B outside the narrow form (the small / mid forms, N < 16, forced forms):
  // one element per lane over 16 lanes (+9% against 4 lanes of float4 in the round-2 bandwidth
  // configuration, scripts/ab.py); wider rows keep the widest vector
  // 16-bit rows of at most 128 B (N <= 64) in the bandwidth configuration: at least 16 lanes per
  // row (VEC = N / 16: 2-8 B per lane) instead of the widest vector over 4-8 lanes; products bf16
  // N = 8 / 16 / 32 / 64 -8 / -7 / -6 / -13%, Reddit-shaped N = 16 / 32 / 64 -27 / -19 / -6%
  // (profiles/r03y_lanes_*.jsonl; fp32 keeps its layouts, DESIGN.md §3 tuning record)
  // The prefetching form too (mid-size graphs): arxiv-shaped bf16 N = 16 took 214 us with 8-element
  // lanes (two active lanes per 4-lane group) against 49 us for fp32 (profiles/r03ah_*.jsonl).
  // The small and mid forms too (round 4, profiles/r04y_small16.jsonl, interleaved A/B): PubMed-
  // shaped bf16 / f16 N = 8-32 33 -> 23 us, N = 64 36 -> 29; 20k rows x 400k N = 8-64 -4..-30%;
  // Cora-shaped (host-bound) -1..-8%.
  const bool narrow16 = !forced_vec && sizeof(T) == 2 && L.n <= 64 && variant == 0;
  int cap16 = 1;  // the largest power of two <= N / 16
  while (cap16 * 32 <= L.n) cap16 *= 2;
  const int vec = (!forced_vec && sizeof(T) == 4 && L.n <= 16) ? 1
                  : narrow16 ? pick_vec((int)sizeof(T), L, 0, cap16)
                             : pick_vec((int)sizeof(T), L, forced_vec);
  OFX_REQUIRE(vec > 0, OFX_EINVAL,
              "spmm_csr: variant %d not applicable (n=%lld ldb=%lld ldc=%lld or pointer alignment)",
              variant, (long long)L.n, (long long)L.ldb, (long long)L.ldc);
  int lpr = forced_lpr ? forced_lpr : pick_lpr(L.n, vec);
  // rows of fewer than 8 single-element lanes in the bandwidth configuration: 8-lane groups (idle
  // lanes included), not 4-lane ones; fp32 N = 1 / 2 / 3 / 4 on products -11 / -9 / -8 / -9%, on
  // the 1M power-law graph N = 1 / 4 -10 / -22%.  16 lanes won on products at N = 2-8 by 2-8% but
  // lost on the power-law graph by 4-48% (profiles/r03af_sweep.jsonl)
  if (!forced_lpr && vec == 1 && lpr < 8 && variant == 0 && form == Form::Bandwidth) lpr = 8;
  switch (vec) {
    case 1: return launch_vec<T, I, 1>(L, form, x, lpr, nt);
    case 2: return launch_vec<T, I, 2>(L, form, x, lpr, nt);
    case 4:
      if constexpr (sizeof(T) <= 4) return launch_vec<T, I, 4>(L, form, x, lpr, nt);
      break;
    case 8:
      if constexpr (sizeof(T) == 2) return launch_vec<T, I, 8>(L, form, x, lpr, nt);
      break;
  }
  return fail(OFX_EINVAL, "spmm_csr: unsupported vector width %d", vec);
}

}  // namespace ofx

#define OFX_SPMM_INSTANTIATE(T, I) template int ofx::launch_typed<T, I>(const ofx::Launch& L);

#endif  // OFX_SPMM_FORWARD_RULES_H_
