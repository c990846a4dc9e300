// spdp_wave.h -- the wave-level primitives of the kernels, each once (device only): moves between lanes, the loads and
// stores of arrays that may cross CUs, the named waits, and the small score arithmetic every engine repeats.  These are
// the lines where the coherence rules live -- which scope, which wait -- so a kernel names them and does not spell them.
#ifndef SPDP_WAVE_H
#define SPDP_WAVE_H
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "spdp_dev.h"

// ---- moves between lanes.  A DPP row is 16 lanes: one stripe of the sweeps.
#define DPP_ROW_SL(n) (0x100 + (n))
#define DPP_ROW_SR(n) (0x110 + (n))
#define DPP_ROW_RR(n) (0x120 + (n))
#define DPP_WAVE_SR1 0x138
// lane i of every 16-lane row <- lane i - 1; lane 0 of the row keeps `old`
__device__ __forceinline__ int row_shr1(int old, int src) { return __builtin_amdgcn_update_dpp(old, src, DPP_ROW_SR(1), 0xf, 0xf, false); }
__device__ __forceinline__ float row_shr1(float old, float src) { return __int_as_float(row_shr1(__float_as_int(old), __float_as_int(src))); }
// lane i of the wave <- lane i - 1; lane 0 keeps `old`
__device__ __forceinline__ int wave_shr1(int old, int src) { return __builtin_amdgcn_update_dpp(old, src, DPP_WAVE_SR1, 0xf, 0xf, false); }
// The two below say bound_ctrl, the moves above must not: only lane 0 of a row is looked at here and it always has a
// source lane, so no `old` operand has to be kept alive; above, `old` is the point.
// lane 0 of every row <- lane J of that row (other lanes: don't care)
template <int J> __device__ __forceinline__ int row_pick(int src)
{
    if constexpr (J == 0) return src;
    else return __builtin_amdgcn_mov_dpp(src, DPP_ROW_SL(J), 0xf, 0xf, true);
}
// lane 0 of every row <- lane 15 of that row
__device__ __forceinline__ int row_ror1(int src) { return __builtin_amdgcn_mov_dpp(src, DPP_ROW_RR(1), 0xf, 0xf, true); }
// lane k <- lane k - 1 of its 16-lane group (through LDS hardware: where the value is not wave-shaped enough for DPP)
__device__ __forceinline__ int up16(int v) { return __shfl_up(v, 1, 16); }
__device__ __forceinline__ int lane_id() { return (int) threadIdx.x; }      // (kernels of one wave per block)
// inclusive scans over the 64 lanes of a wave; lane: the caller's lane in its wave
__device__ __forceinline__ int wave_scan_add(int v, int lane)
{
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const int u = __shfl_up(v, d); if (lane >= d) v += u; }
    return v;
}
__device__ __forceinline__ int wave_scan_max(int v, int lane)
{
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const int u = __shfl_up(v, d); if (lane >= d) v = max(v, u); }
    return v;
}

// a problem record every lane has read from the same address: its words, said to be wave-uniform, live in SGPRs -- and so
// does everything computed from them (ranges, array bases, loop bounds)
template <class T> __device__ __forceinline__ T wave_uniform(const T& t)
{
    static_assert(sizeof(T) % 4 == 0, "words");
    T r;
    const int* src = reinterpret_cast<const int*>(&t);
    int* dst = reinterpret_cast<int*>(&r);
#pragma unroll
    for (unsigned i = 0; i < sizeof(T) / 4; ++i) dst[i] = __builtin_amdgcn_readfirstlane(src[i]);
    return r;
}

// ---- ordering inside ONE wave needs no hardware fence: a wave's LDS instructions execute in order, and so do its
// vector-memory instructions (a load issued after a store of the same wave to the same address observes it).  Only the
// compiler must not move accesses across these points.  (A wavefront-scope __builtin_amdgcn_fence would do, but it makes
// the compiler wait for all loads right after a prefetch -- no prefetch left.)
#define WAVE_ORDER() asm volatile("" ::: "memory")
// the named waits: this wave's stores have reached memory (what a progress word may be published after) or, the same
// wait, its loads have arrived; its LDS traffic is done; both -- and the latter two with the wave barrier that also
// keeps the compiler from moving cross-lane operations over them
__device__ __forceinline__ void stores_drained() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }
__device__ __forceinline__ void loads_arrived() { stores_drained(); }        // (one counter for vector loads and stores alike)
__device__ __forceinline__ void lds_done() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }
__device__ __forceinline__ void mem_done() { asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory"); }
__device__ __forceinline__ void lds_sync() { lds_done(); __builtin_amdgcn_wave_barrier(); }
__device__ __forceinline__ void wave_sync() { mem_done(); __builtin_amdgcn_wave_barrier(); }

// ---- loads that bypass the L1: data another row of this wave stored a few blocks ago
typedef int v4i_t __attribute__((ext_vector_type(4)));
typedef int v2i_t __attribute__((ext_vector_type(2)));
__device__ __forceinline__ int4 ld_nt4(const int* p)
{
    const v4i_t v = __builtin_nontemporal_load(reinterpret_cast<const v4i_t*>(p));
    return make_int4(v.x, v.y, v.z, v.w);
}
__device__ __forceinline__ int2 ld_nt2(const int* p)
{
    const v2i_t v = __builtin_nontemporal_load(reinterpret_cast<const v2i_t*>(p));
    return make_int2(v.x, v.y);
}
__device__ __forceinline__ int4 ld_nt4(const int4* p) { return ld_nt4(reinterpret_cast<const int*>(p)); }
__device__ __forceinline__ int2 ld_nt2(const int2* p) { return ld_nt2(reinterpret_cast<const int*>(p)); }
__device__ __forceinline__ int ld_nt1(const int* p) { return __builtin_nontemporal_load(p); }
__device__ __forceinline__ unsigned ld_nt_u16(const uint16_t* p) { return __builtin_nontemporal_load(p); }

// ---- boundary / diagonal arrays.  X: the array crosses CUs (a problem's stripes or tiles run as separate waves).  The
// per-XCD L2s are not coherent with each other, so every access then goes to the memory side -- agent-scope relaxed
// atomics compile to sc1 loads / stores (write-through, no allocation of stale lines); a progress word published after
// stores_drained() orders them for the consumer.  Otherwise: L1-bypassing loads, plain stores.
template <bool X> __device__ __forceinline__ int gld(const int* p)
{
    if constexpr (X) return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else return __builtin_nontemporal_load(p);
}
// ... with a plain load where nothing crosses: spdh_exact<., false> reads back, stripe after stripe, what its own group
// stored, and was tuned with these reads served from the L1
template <bool X> __device__ __forceinline__ int gld_l1(const int* p)
{
    if constexpr (X) return gld<true>(p);
    else return *p;
}
template <bool X> __device__ __forceinline__ void gst(int* p, int v)
{
    if constexpr (X) __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else *p = v;
}
template <bool X> __device__ __forceinline__ int4 ld_b4(const int* p)
{
    if constexpr (X) return make_int4(gld<true>(p), gld<true>(p + 1), gld<true>(p + 2), gld<true>(p + 3));
    else return ld_nt4(p);
}
template <bool X> __device__ __forceinline__ int2 ld_b2(const int* p)
{
    if constexpr (X) return make_int2(gld<true>(p), gld<true>(p + 1));
    else return ld_nt2(p);
}
template <bool X> __device__ __forceinline__ void st_b4(int* p, int4 v)
{
    if constexpr (X) { gst<true>(p, v.x); gst<true>(p + 1, v.y); gst<true>(p + 2, v.z); gst<true>(p + 3, v.w); }
    else *reinterpret_cast<int4*>(p) = v;
}
template <bool X> __device__ __forceinline__ void st_b2(int* p, int2 v)
{
    if constexpr (X) { gst<true>(p, v.x); gst<true>(p + 1, v.y); }
    else *reinterpret_cast<int2*>(p) = v;
}
// N entries of arrays that cross CUs at once: the agent-scope atomic load the compiler emits for each entry is followed
// by a wait of its own -- a refill of ten planes was ten memory round trips in a row.  The same loads (sc1: the memory
// side, past the non-coherent L2s) issued together, one wait.  The compiler does not know these loads are
// asynchronous: nothing may look at v[] before the wait, which the empty statements behind it see to.
template <bool X, int N>
__device__ __forceinline__ void gld_n(const int* const (&base)[N], int e, int (&v)[N])      // v[i] = base[i][e], base[] wave-uniform
{
    if constexpr (X) {
        const unsigned off = (unsigned) e * 4u;
#pragma unroll
        for (int i = 0; i < N; ++i) {
            asm volatile("global_load_dword %0, %1, %2 sc1" : "=v"(v[i]) : "v"(off), "s"(base[i]));
        }
        loads_arrived();
#pragma unroll
        for (int i = 0; i < N; ++i) asm volatile("" : "+v"(v[i]));
    } else {
#pragma unroll
        for (int i = 0; i < N; ++i) v[i] = __builtin_nontemporal_load(base[i] + e);
    }
}

// ---- score arithmetic
// int16 scores held in ints: an add that saturates at the floor only (the sweeps never reach the ceiling)
__device__ __forceinline__ int sadd16(int a, int b) { return max(a + b, SPDP_FLOOR16); }
// int16 scores proper, and int16 scores in the UPPER half of 32-bit registers (value * 65536): `v_add_i32 ... clamp` then
// saturates exactly where `v_add_i16 ... clamp` does, at less than half the issue cost (profiles/r02_valu_ubench.txt:
// 7.7 cycles per wave-instruction for the 16-bit VOP3 form, 4 for the 32-bit one), and order comparisons are unchanged
typedef short s16;
typedef int q16;
#define Q16(x) ((q16) ((unsigned) (x) << 16))
__device__ __forceinline__ s16 sadd(s16 a, s16 b) { return __builtin_elementwise_add_sat(a, b); }
__device__ __forceinline__ s16 smax(s16 a, s16 b) { return a > b ? a : b; }
__device__ __forceinline__ q16 qadd(q16 a, q16 b) { return __builtin_elementwise_add_sat(a, b); }
__device__ __forceinline__ q16 qmax(q16 a, q16 b) { return a > b ? a : b; }
// post-splice flag of a state (src/aln.h:56): H 4, E 1, F 8, E2 2, F2 16 -- arithmetic, not a table in memory
__device__ __forceinline__ int psp_bit(int k) { return k == 0 ? 4 : (k == 1 ? 1 : (k == 2 ? 8 : (k == 3 ? 2 : 16))); }
// ... of the engines that have three states only: two compares less, and any k >= 2 is F
__device__ __forceinline__ int psp_bit3(int k) { return k == 0 ? 4 : (k == 1 ? 1 : 8); }

#endif
