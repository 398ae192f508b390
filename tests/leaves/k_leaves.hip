// TEST INFRASTRUCTURE -- the leaf bench: k_map's sort, merge and repair leaves and the wave primitives, each behind a kernel that
// calls that one leaf and nothing else, on inputs the test chose.  Never part of the package: tests/leaves_lib.py builds it for
// gfx950, tests/lanesim/Makefile.leaves for the emulator.  The headers come in the order k_map.hip includes them (map_lds.h
// defines the s_e the merges stage in).
//
// One launch carries many cases: workgroup b (one wavefront) reads descriptor b and works in its own slot, slots + b * slot_bytes.
// A descriptor is LEAF_DESC_WORDS 32-bit words (tests/leaves_cases.py writes them by the same names):
//    0.. 5  A.adj     6..11  A.cum    12  A.n          a KeyArr of up to six runs
//   13..16  B.adj    17..20  B.cum    21  B.n          a second one of up to four
//   22      out_off                                    byte offset of the output in the slot
//   23..29  p0..p6                                     what else the leaf takes
//   30, 31  ret                                        what it returned (64 bits, low word first)
// To add a leaf: a kernel below that unpacks what it needs and calls it, a line in leaves_run's switch, its number in
// tests/leaves_cases.py.  Plain C++ stores only.
#include <hip/hip_runtime.h>

#include <type_traits>
#include <vector>

#include "unc_dev_types.h"
#include "wave_prims.h"

#include "map_lds.h"
#include "map_sort.h"
#include "map_sort_wide.h"

using namespace unc;

constexpr uint32_t LEAF_DESC_WORDS = 32;
enum { D_AADJ = 0, D_ACUM = 6, D_AN = 12, D_BADJ = 13, D_BCUM = 17, D_BN = 21, D_OUT = 22, D_P = 23, D_RET = 30 };

struct LeafCtx {
    uint32_t *d;        // this case's descriptor
    gptr_t sb;          // this case's slot
    int lane;
};
__device__ __forceinline__ LeafCtx leaf_ctx(uint32_t *desc, char *slots, uint64_t slot_bytes) {
    LeafCtx c;
    c.d = desc + (size_t)blockIdx.x * LEAF_DESC_WORDS;
    c.sb = (gptr_t)(slots + (size_t)blockIdx.x * slot_bytes);
    c.lane = lane_id();
    return c;
}
template <int R> __device__ __forceinline__ KeyArr<R> leaf_A(const uint32_t *d) {
    KeyArr<R> K;
#pragma unroll
    for (int r = 0; r < R; ++r) { K.adj[r] = d[D_AADJ + r]; K.cum[r] = d[D_ACUM + r]; }
    K.n = d[D_AN];
    return K;
}
template <int R> __device__ __forceinline__ KeyArr<R> leaf_B(const uint32_t *d) {
    KeyArr<R> K;
#pragma unroll
    for (int r = 0; r < R; ++r) { K.adj[r] = d[D_BADJ + r]; K.cum[r] = d[D_BCUM + r]; }
    K.n = d[D_BN];
    return K;
}
__device__ __forceinline__ void leaf_ret(const LeafCtx &c, uint64_t v) {
    if (c.lane == 0) { c.d[D_RET] = (uint32_t)v; c.d[D_RET + 1] = (uint32_t)(v >> 32); }
}

// ---- wave primitives.  Slot: v[64] u64 at 0, h[64] u32 at 512, out0[64] u64 at 768, out1[64] u64 at 1280.  p0 = primitive, p1 = its parameter
enum { WP_SEG64 = 0, WP_SEG32, WP_SUMB2, WP_SUMB3, WP_SUMB7, WP_SUM32, WP_MAX32, WP_POPC, WP_WSUM64, WP_BCAST64, WP_BCAST32, WP_UNIFORM64, WP_BCASTF };
extern "C" __global__ __launch_bounds__(64) void leaf_wave_prims(uint32_t *desc, char *slots, uint64_t slot_bytes) {
    const LeafCtx c = leaf_ctx(desc, slots, slot_bytes);
    const uint32_t prim = uniform32(c.d[D_P]), par = uniform32(c.d[D_P + 1]);
    const uint32_t l = (uint32_t)c.lane;
    const uint64_t v = gld<uint64_t>(c.sb, l << 3);
    const uint32_t h = gld<uint32_t>(c.sb, 512u + (l << 2));
    uint64_t o0 = 0, o1 = 0;
    uint32_t tot = 0;
    switch (prim) {
    case WP_SEG64: o0 = par ? seg_incl_max64(v, c.lane == 0) : seg_incl_max64(v, h != 0u); break;      // (par: the repair's call; else the walk's)
    case WP_SEG32: o0 = par ? seg_incl_max32((uint32_t)v, c.lane == 0) : seg_incl_max32((uint32_t)v, h != 0u); break;
    case WP_SUMB2: o0 = excl_sum_bits<2>((uint32_t)v, &tot); o1 = tot; break;
    case WP_SUMB3: o0 = excl_sum_bits<3>((uint32_t)v, &tot); o1 = tot; break;
    case WP_SUMB7: o0 = excl_sum_bits<7>((uint32_t)v, &tot); o1 = tot; break;
    case WP_SUM32: o0 = excl_sum32((uint32_t)v, &tot); o1 = tot; break;
    case WP_MAX32: o0 = excl_max32((uint32_t)v, &tot); o1 = tot; break;
    case WP_POPC: o0 = prefix_popc(gld<uint64_t>(c.sb, 0u)); break;            // (the mask is uniform: every lane reads v[0])
    case WP_WSUM64: o0 = wave_sum64(v); break;
    case WP_BCAST64: o0 = bcast64(v, (int)par); break;
    case WP_BCAST32: o0 = bcast32((uint32_t)v, (int)par); break;
    case WP_UNIFORM64: o0 = uniform64(v); break;
    case WP_BCASTF: o0 = __float_as_uint(bcastf(__uint_as_float((uint32_t)v), (int)par)); break;
    default: break;
    }
    gst(c.sb, 768u + (l << 3), o0);
    gst(c.sb, 1280u + (l << 3), o1);
}

// ---- narrow sorts: A = the KeyArr<6>, out_off; p0 = 0: sort_any64, 1 / 2 / 4 / 8: sort_regs64<p0>, 9: sort_hybrid64
extern "C" __global__ __launch_bounds__(64) void leaf_sort64(uint32_t *desc, char *slots, uint64_t slot_bytes) {
    const LeafCtx c = leaf_ctx(desc, slots, slot_bytes);
    const KeyArr<6> K = leaf_A<6>(c.d);
    const uint32_t out_off = c.d[D_OUT];
    switch (uniform32(c.d[D_P])) {
    case 0: sort_any64(c.sb, K, out_off, c.lane); break;
    case 1: sort_regs64<1>(c.sb, K, out_off, c.lane); break;
    case 2: sort_regs64<2>(c.sb, K, out_off, c.lane); break;
    case 4: sort_regs64<4>(c.sb, K, out_off, c.lane); break;
    case 8: sort_regs64<8>(c.sb, K, out_off, c.lane); break;
    case 9: sort_hybrid64(c.sb, K, out_off, c.lane); break;
    default: break;
    }
}

// ---- legacy 128-bit sorts: in = A.adj[0], n = A.n, out_off; p0 = 1 / 2 / 4 / 8: sort_regs<p0>, 9: sort_hybrid
extern "C" __global__ __launch_bounds__(64) void leaf_sort128(uint32_t *desc, char *slots, uint64_t slot_bytes) {
    const LeafCtx c = leaf_ctx(desc, slots, slot_bytes);
    const UNC_AS_GLOBAL SortKey *const in = reinterpret_cast<const UNC_AS_GLOBAL SortKey *>(c.sb + c.d[D_AADJ]);
    UNC_AS_GLOBAL SortKey *const out = reinterpret_cast<UNC_AS_GLOBAL SortKey *>(c.sb + c.d[D_OUT]);
    const uint32_t n = c.d[D_AN];
    switch (uniform32(c.d[D_P])) {
    case 1: sort_regs<1>(in, out, n, c.lane); break;
    case 2: sort_regs<2>(in, out, n, c.lane); break;
    case 4: sort_regs<4>(in, out, n, c.lane); break;
    case 8: sort_regs<8>(in, out, n, c.lane); break;
    case 9: sort_hybrid(in, out, n, c.lane); break;
    default: break;
    }
}

// ---- merges: A, B, out_off; p0 = verify (narrow).  ret = what merge_runs returned
extern "C" __global__ __launch_bounds__(64) void leaf_merge41(uint32_t *desc, char *slots, uint64_t slot_bytes) {
    const LeafCtx c = leaf_ctx(desc, slots, slot_bytes);
    leaf_ret(c, merge_runs<4, 1>(c.sb, leaf_A<4>(c.d), leaf_B<1>(c.d), c.d[D_OUT], c.lane, c.d[D_P]));
}
extern "C" __global__ __launch_bounds__(64) void leaf_merge14(uint32_t *desc, char *slots, uint64_t slot_bytes) {
    const LeafCtx c = leaf_ctx(desc, slots, slot_bytes);
    leaf_ret(c, merge_runs<1, 4>(c.sb, leaf_A<1>(c.d), leaf_B<4>(c.d), c.d[D_OUT], c.lane, c.d[D_P]));
}
extern "C" __global__ __launch_bounds__(64) void leaf_mergew41(uint32_t *desc, char *slots, uint64_t slot_bytes) {
    const LeafCtx c = leaf_ctx(desc, slots, slot_bytes);
    mergew_runs<4, 1>(c.sb, leaf_A<4>(c.d), leaf_B<1>(c.d), c.d[D_OUT], c.lane);
}

// ---- the splits alone: p0 = 0: merge_split<4,1>, 1: merge_split<1,4>, 2: mergew_split<4,1>; p1 = byte offset of the diagonals (u32), p2 = how
// many; the split of diagonal j goes to out_off + 4 j
extern "C" __global__ __launch_bounds__(64) void leaf_split(uint32_t *desc, char *slots, uint64_t slot_bytes) {
    const LeafCtx c = leaf_ctx(desc, slots, slot_bytes);
    const uint32_t which = uniform32(c.d[D_P]), d_off = uniform32(c.d[D_P + 1]), nd = uniform32(c.d[D_P + 2]), out_off = uniform32(c.d[D_OUT]);
    const KeyArr<4> A4 = ka_uniform(leaf_A<4>(c.d));
    const KeyArr<1> B1 = ka_uniform(leaf_B<1>(c.d));
    const KeyArr<1> A1 = ka_uniform(leaf_A<1>(c.d));
    const KeyArr<4> B4 = ka_uniform(leaf_B<4>(c.d));
    for (uint32_t j = 0; j < nd; ++j) {
        const uint32_t d = uniform32(gld<uint32_t>(c.sb, d_off + (j << 2)));
        uint32_t s;
        if (which == 0u) s = merge_split(c.sb, A4, B1, d, c.lane);
        else if (which == 1u) s = merge_split(c.sb, A1, B4, d, c.lane);
        else s = mergew_split(c.sb, A4, B1, d, c.lane);
        if (c.lane == 0) gst(c.sb, out_off + (j << 2), s);
    }
}

// ---- one tile staged: p0 = 0: stage_tile<4,1>, 1: stage_tile<1,4>, 2: stagew_tile<4,1> followed by mergew_tile; p1 = a0, p2 = b0, p3 = na,
// p4 = nb.  The tile's keys leave LDS for out_off in tile order (0 / 1: as staged, A's share then B's; 2: merged)
extern "C" __global__ __launch_bounds__(64) void leaf_tile(uint32_t *desc, char *slots, uint64_t slot_bytes) {
    const LeafCtx c = leaf_ctx(desc, slots, slot_bytes);
    const uint32_t which = uniform32(c.d[D_P]), a0 = uniform32(c.d[D_P + 1]), b0 = uniform32(c.d[D_P + 2]), na = uniform32(c.d[D_P + 3]),
                   nb = uniform32(c.d[D_P + 4]), out_off = uniform32(c.d[D_OUT]);
    const uint32_t tn = na + nb;
    if (which <= 1u) {
        if (which == 0u) stage_tile(c.sb, ka_uniform(leaf_A<4>(c.d)), ka_uniform(leaf_B<1>(c.d)), a0, b0, na, tn, s_e, c.lane);
        else stage_tile(c.sb, ka_uniform(leaf_A<1>(c.d)), ka_uniform(leaf_B<4>(c.d)), a0, b0, na, tn, s_e, c.lane);
        wave_sync();
        // (the tile's layout in LDS restated, not taken from mslot: one pad slot per 8 keys.  The walk and the team kernels read tiles staged
        // by this leaf with that layout; a change of it shows here)
        for (uint32_t i = (uint32_t)c.lane; i < tn; i += WAVE) gst(c.sb, out_off + (i << 3), s_e[i + (i >> 3)]);
    } else {
        SortKey *const tile = reinterpret_cast<SortKey *>(s_e);
        stagew_tile(c.sb, ka_uniform(leaf_A<4>(c.d)), ka_uniform(leaf_B<1>(c.d)), a0, b0, na, tn, tile, c.lane);
        wave_sync();
        SortKey o[MERGEW_C];
        uint32_t d, cnt;
        mergew_tile(tile, na, nb, c.lane, o, d, cnt);
        wave_sync();
#pragma unroll
        for (uint32_t k = 0; k < MERGEW_C; ++k)
            if (k < cnt) gst(c.sb, out_off + ((d + k) << 4), o[k]);
    }
}

// ---- repairs.  run: run_off = A.adj[0], n = A.n, x_off = out_off, nx = p0 (p1 = 1: the wide one).  runs4: str_off = A.adj[0], run_bytes = p1,
// n1..n4 = A.cum[0..3], x_off = out_off, nx = p0.  ret = what the leaf returned
extern "C" __global__ __launch_bounds__(64) void leaf_repair_run(uint32_t *desc, char *slots, uint64_t slot_bytes) {
    const LeafCtx c = leaf_ctx(desc, slots, slot_bytes);
    if (uniform32(c.d[D_P + 1])) leaf_ret(c, repairw_run(c.sb, c.d[D_AADJ], c.d[D_AN], c.d[D_OUT], c.d[D_P], c.lane));
    else leaf_ret(c, repair_run(c.sb, c.d[D_AADJ], c.d[D_AN], c.d[D_OUT], c.d[D_P], c.lane));
}
extern "C" __global__ __launch_bounds__(64) void leaf_repair_runs4(uint32_t *desc, char *slots, uint64_t slot_bytes) {
    const LeafCtx c = leaf_ctx(desc, slots, slot_bytes);
    leaf_ret(c, repair_runs4(c.sb, c.d[D_AADJ], c.d[D_P + 1], c.d[D_ACUM], c.d[D_ACUM + 1], c.d[D_ACUM + 2], c.d[D_ACUM + 3], c.d[D_OUT], c.d[D_P], c.lane));
}

// ---- phase S's chain at the leaf level, in phase_S's offsets and KeyArrs (k_map.hip, phase_S: the arithmetic of KM and KB is copied from it).
// str_off = A.adj[0], run_bytes = p1, scnt1..4 = A.cum[0..3], nx = p0, off_tmp (narrow) / ukeys_off (wide) = out_off, skeys_off = p2 (wide),
// p3 = 1: wide.  ret = KB.n | KB.adj[0] << 32: where the merged moves-and-unsorted sequence lies; p4..p6 and A.n take scnt1..4 after the repair
extern "C" __global__ __launch_bounds__(64) void leaf_chain(uint32_t *desc, char *slots, uint64_t slot_bytes) {
    const LeafCtx c = leaf_ctx(desc, slots, slot_bytes);
    const gptr_t sb = c.sb;
    const int lane = c.lane;
    const uint32_t str_off = uniform32(c.d[D_AADJ]), run_bytes = uniform32(c.d[D_P + 1]), off_out = uniform32(c.d[D_OUT]), skeys_off = uniform32(c.d[D_P + 2]);
    const bool wide = uniform32(c.d[D_P + 3]) != 0u;
    uint32_t scnt1 = uniform32(c.d[D_ACUM]), scnt2 = uniform32(c.d[D_ACUM + 1]), scnt3 = uniform32(c.d[D_ACUM + 2]), scnt4 = uniform32(c.d[D_ACUM + 3]);
    uint32_t nx = uniform32(c.d[D_P]);
    const uint32_t x_off = str_off + 5u * run_bytes;
    const uint32_t sh = wide ? 4u : 3u;
    uint32_t xs_off = x_off;
    wave_sync();
    if (!wide) {
        if (scnt1 > 1 || scnt2 > 1 || scnt3 > 1 || scnt4 > 1) {
            const uint64_t v4 = repair_runs4(sb, str_off, run_bytes, scnt1, scnt2, scnt3, scnt4, x_off, nx, lane);
            const uint32_t v1 = (uint32_t)v4 & 0xFFFFu, v2 = (uint32_t)(v4 >> 16) & 0xFFFFu, v3 = (uint32_t)(v4 >> 32) & 0xFFFFu, v4r = (uint32_t)(v4 >> 48);
            scnt1 -= v1; scnt2 -= v2; scnt3 -= v3; scnt4 -= v4r; nx += v1 + v2 + v3 + v4r;
        }
        wave_sync();
        if (nx > 1) {
            KeyArr<6> KX;
#pragma unroll
            for (int r = 0; r < 6; ++r) { KX.adj[r] = x_off; KX.cum[r] = 0; }
            KX.n = nx;
            sort_any64(sb, KX, x_off, lane);          // in place
            wave_sync();
        }
    } else {
        if (scnt1 > 1) { const uint32_t v = repairw_run(sb, str_off + run_bytes, scnt1, x_off, nx, lane); scnt1 -= v; nx += v; }
        if (scnt2 > 1) { const uint32_t v = repairw_run(sb, str_off + 2u * run_bytes, scnt2, x_off, nx, lane); scnt2 -= v; nx += v; }
        if (scnt3 > 1) { const uint32_t v = repairw_run(sb, str_off + 3u * run_bytes, scnt3, x_off, nx, lane); scnt3 -= v; nx += v; }
        if (scnt4 > 1) { const uint32_t v = repairw_run(sb, str_off + 4u * run_bytes, scnt4, x_off, nx, lane); scnt4 -= v; nx += v; }
        wave_sync();
        if (nx > 1) {
            const UNC_AS_GLOBAL SortKey *const xin = reinterpret_cast<const UNC_AS_GLOBAL SortKey *>(sb + x_off);
            UNC_AS_GLOBAL SortKey *const skeys = reinterpret_cast<UNC_AS_GLOBAL SortKey *>(sb + skeys_off);
            if (nx <= 64) sort_regs<1>(xin, skeys, nx, lane);
            else if (nx <= 128) sort_regs<2>(xin, skeys, nx, lane);
            else if (nx <= 256) sort_regs<4>(xin, skeys, nx, lane);
            else if (nx <= 512) sort_regs<8>(xin, skeys, nx, lane);
            else sort_hybrid(xin, skeys, nx, lane);
            xs_off = skeys_off;
            wave_sync();
        }
    }
    KeyArr<4> KM;       // the moves, base by base
    KM.cum[0] = 0; KM.cum[1] = scnt1; KM.cum[2] = scnt1 + scnt2; KM.cum[3] = scnt1 + scnt2 + scnt3;
    KM.n = KM.cum[3] + scnt4;
#pragma unroll
    for (uint32_t r = 0; r < 4; ++r) KM.adj[r] = str_off + (r + 1u) * run_bytes - (KM.cum[r] << sh);
    KeyArr<4> KB = KM;
    if (nx > 0) {
        if (KM.n > 0) {
            if (!wide) merge_runs<4, 1>(sb, KM, ka_single(xs_off, nx), off_out, lane, 0u);
            else mergew_runs<4, 1>(sb, KM, kaw_single(xs_off, nx), off_out, lane);
            wave_sync();
            KB.adj[0] = off_out;
        } else KB.adj[0] = xs_off;
        KB.cum[1] = KB.cum[2] = KB.cum[3] = KB.n = KM.n + nx;
        KB.adj[1] = KB.adj[2] = KB.adj[3] = KB.adj[0];
    }
    if (lane == 0) { c.d[D_P + 4] = scnt1; c.d[D_P + 5] = scnt2; c.d[D_P + 6] = scnt3; c.d[D_AN] = scnt4; }
    leaf_ret(c, (uint64_t)KB.n | ((uint64_t)KB.adj[0] << 32));
}

// ---- host side: descriptors and slots in, one launch of `kernel`, both back.  Returns the hipError_t; -2 when the launch wrote behind its
// last slot (the allocation ends with one more slot's worth of 0xA5 bytes, looked at afterwards: a leaf that overruns the last case's
// slot fails its test instead of corrupting the heap)
enum { LK_WAVE = 0, LK_SORT64, LK_SORT128, LK_MERGE41, LK_MERGE14, LK_MERGEW41, LK_SPLIT, LK_TILE, LK_REPAIR_RUN, LK_REPAIR_RUNS4, LK_CHAIN };

extern "C" int leaves_run(int kernel, uint32_t *desc, uint32_t ncases, char *slots, uint64_t slot_bytes) {
    if (!desc || !slots || ncases == 0 || slot_bytes == 0 || (slot_bytes & 15u)) return -1;
    uint32_t *d_desc = nullptr;
    char *d_slots = nullptr;
    const size_t desc_bytes = (size_t)ncases * LEAF_DESC_WORDS * sizeof(uint32_t), slots_bytes = (size_t)ncases * slot_bytes;
    hipError_t e = hipMalloc((void **)&d_desc, desc_bytes);
    if (e == hipSuccess) e = hipMalloc((void **)&d_slots, slots_bytes + slot_bytes);
    if (e == hipSuccess) e = hipMemset(d_slots + slots_bytes, 0xA5, slot_bytes);
    if (e == hipSuccess) e = hipMemcpy(d_desc, desc, desc_bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_slots, slots, slots_bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        const dim3 grid(ncases), block(64);
        switch (kernel) {
        case LK_WAVE: hipLaunchKernelGGL(leaf_wave_prims, grid, block, 0, 0, d_desc, d_slots, slot_bytes); break;
        case LK_SORT64: hipLaunchKernelGGL(leaf_sort64, grid, block, 0, 0, d_desc, d_slots, slot_bytes); break;
        case LK_SORT128: hipLaunchKernelGGL(leaf_sort128, grid, block, 0, 0, d_desc, d_slots, slot_bytes); break;
        case LK_MERGE41: hipLaunchKernelGGL(leaf_merge41, grid, block, 0, 0, d_desc, d_slots, slot_bytes); break;
        case LK_MERGE14: hipLaunchKernelGGL(leaf_merge14, grid, block, 0, 0, d_desc, d_slots, slot_bytes); break;
        case LK_MERGEW41: hipLaunchKernelGGL(leaf_mergew41, grid, block, 0, 0, d_desc, d_slots, slot_bytes); break;
        case LK_SPLIT: hipLaunchKernelGGL(leaf_split, grid, block, 0, 0, d_desc, d_slots, slot_bytes); break;
        case LK_TILE: hipLaunchKernelGGL(leaf_tile, grid, block, 0, 0, d_desc, d_slots, slot_bytes); break;
        case LK_REPAIR_RUN: hipLaunchKernelGGL(leaf_repair_run, grid, block, 0, 0, d_desc, d_slots, slot_bytes); break;
        case LK_REPAIR_RUNS4: hipLaunchKernelGGL(leaf_repair_runs4, grid, block, 0, 0, d_desc, d_slots, slot_bytes); break;
        case LK_CHAIN: hipLaunchKernelGGL(leaf_chain, grid, block, 0, 0, d_desc, d_slots, slot_bytes); break;
        default: e = (hipError_t)1; break;
        }
        if (e == hipSuccess) e = hipGetLastError();
        if (e == hipSuccess) e = hipDeviceSynchronize();
    }
    if (e == hipSuccess) e = hipMemcpy(desc, d_desc, desc_bytes, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(slots, d_slots, slots_bytes, hipMemcpyDeviceToHost);
    bool overrun = false;
    if (e == hipSuccess) {
        std::vector<unsigned char> tail(slot_bytes);
        e = hipMemcpy(tail.data(), d_slots + slots_bytes, slot_bytes, hipMemcpyDeviceToHost);
        for (size_t i = 0; e == hipSuccess && i < tail.size(); ++i) overrun = overrun || tail[i] != 0xA5;
    }
    (void)hipFree(d_desc);
    (void)hipFree(d_slots);
    return e != hipSuccess ? (int)e : overrun ? -2 : 0;
}
