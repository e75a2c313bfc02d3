// scan_device.h — the scan toolkit of the query-independent kernels (aot_kernels.hip, devtail.hip): one wave ladder, one workgroup
// scan, one batched single-workgroup scan and one decoupled look-back, each written once.  Device code only; the pipeline kernels
// that hiprtc compiles have their own header (kernels/rsq_device.h) and do not see this one.
//
// An operator is a struct with identity(), apply(a, b) and the constant `invertible`: ScanSum over unsigned / u64, ScanMin over i64.
// `invertible` says whether what lies in front of a lane can be had as (inclusive value - own value); block_scan asks the lane in front
// otherwise (one more shuffle).
#pragma once

#include <hip/hip_runtime.h>

namespace rsq {

typedef long long i64;
typedef unsigned long long u64;

// ---- geometry -----------------------------------------------------------------------------------------------------------------
#define SCAN_BATCH 1024          /* values per batch of batched_exclusive_scan (its workgroup size): the chunk totals of the sum scan, the chunk
                                    minima of the running minimum, a column of the partition matrix; also the counts per sub-block of a chunk */
#define SCAN_CHUNK 4096          /* counts per workgroup of the sum scan: four sub-blocks of SCAN_BATCH, four neighbouring counts per thread of each */
#define SM_CHUNK 4096            /* values per workgroup of the running minimum */
#define SM_PER_THREAD 16         /* ... SM_PER_THREAD consecutive ones per thread */
static_assert(SCAN_CHUNK == 4 * SCAN_BATCH && SCAN_BATCH == 256 * 4 && SM_CHUNK == 256 * SM_PER_THREAD, "chunk geometry");
// a look-back gives up after this many ticks of wall_clock64: 100 MHz clock, 1 ms
#define LOOK_BACK_TIMEOUT_TICKS 100000ll

struct ScanSum {
    static __device__ __forceinline__ unsigned identity() { return 0u; }          // (widens to u64 where T is)
    template <typename T> static __device__ __forceinline__ T apply(T a, T b) { return a + b; }
    static constexpr bool invertible = true;           // everything in front of a lane = its inclusive value - its own
};
struct ScanMin {
    static __device__ __forceinline__ i64 identity() { return 0x7fffffffffffffffll; }
    static __device__ __forceinline__ i64 apply(i64 a, i64 b) { return a < b ? a : b; }
    static constexpr bool invertible = false;          // ... a minimum has to ask the lane in front
};

// (a 64-bit value goes through the long long shuffles, a 32-bit one through the int ones)
template <typename T> __device__ __forceinline__ T wave_shfl_up(T x, int d) {
    if constexpr (sizeof(T) == 8) return (T)__shfl_up((long long)x, d, 64); else return (T)__shfl_up((int)x, d, 64);
}
template <typename T> __device__ __forceinline__ T wave_sum(T x) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        if constexpr (sizeof(T) == 8) x += (T)__shfl_xor((long long)x, m, 64); else x += (T)__shfl_xor((int)x, m, 64);
    }
    return x;
}

// inclusive scan over the 64 lanes of a wave: six steps of __shfl_up
template <typename T, typename Op> __device__ __forceinline__ T wave_inclusive_scan(T x) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const T v = wave_shfl_up(x, d); if (lane >= d) x = Op::apply(v, x); }
    return x;
}

// Exclusive prefix of x over a workgroup of THREADS threads, and the workgroup's total: wave scan, then the wave totals through
// s_wave[THREADS / 64].  One barrier.  The LDS is the caller's: whoever calls again before another barrier hands in another array
// (two in turn are enough: a thread that writes set k again has passed the barrier of set k + 1, which every reader of set k reaches
// only after reading).
template <int THREADS, typename T, typename Op> __device__ __forceinline__ T block_scan(T x, T* s_wave, T* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const T incl = wave_inclusive_scan<T, Op>(x);
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    T before = Op::identity(), all = Op::identity();
#pragma unroll 4          // (four totals in flight: sixteen at once cost the 1024-thread scans 32 registers and an occupancy step)
    for (int w = 0; w < THREADS / 64; w++) { const T c = s_wave[w]; if (w < wave) before = Op::apply(before, c); all = Op::apply(all, c); }
    *total = all;
    if constexpr (Op::invertible) return before + (incl - x);
    else { const T up = wave_shfl_up(incl, 1); return lane == 0 ? before : Op::apply(before, up); }
}

// One workgroup of SCAN_BATCH threads scans n values, SCAN_BATCH at a time with a carry: store(i, the exclusive prefix of load(i)).
// Every thread returns the total.  load and store see every i < n once, from the same thread (a scan in place is fine).
template <typename T, typename Op, typename Load, typename Store> __device__ __forceinline__ T batched_exclusive_scan(i64 n, Load load, Store store) {
    __shared__ T s_wave[2][SCAN_BATCH / 64];
    T carry = Op::identity();
    int set = 0;
    for (i64 base = 0; base < n; base += SCAN_BATCH, set ^= 1) {
        const i64 i = base + threadIdx.x;
        const T x = i < n ? (T)load(i) : (T)Op::identity();
        T total;
        const T before = block_scan<SCAN_BATCH, T, Op>(x, s_wave[set], &total);
        if (i < n) store(i, Op::apply(carry, before));
        carry = Op::apply(carry, total);
    }
    return carry;
}

// Decoupled look-back, executed by the FIRST WAVE of workgroup `chunk`: returns the total of all chunks in front of it, every lane.
// chain word = (value << 2) | state: 1 = this chunk's own total, 2 = the total of all chunks up to and including it; `chain` must be
// zero before the launch.  T is unsigned (30 value bits) or u64 (62).
// A chunk publishes its own total at once and then looks BACK over its predecessors, adding own totals until it meets an
// inclusive one: no chunk waits for a chain of 260 hand-overs, which a plain "wait for the chunk before me" turned into 130 us of
// serial latency on TPC-H Q3's 60 M-bit orders bitmap.  The look-back is done by one WAVE, lane l reading the l-th predecessor:
// 64 chain words per round trip (one thread walking them one by one: 19 us for 262 chunks).  Chain words carry their value, so
// relaxed agent-scope loads and stores are all they need.
// Workgroups are dispatched in the order of their index, so whatever a chunk waits for is running or done; a wave that nevertheless
// waits longer than LOOK_BACK_TIMEOUT_TICKS raises stuckBit in *stuck and LEAVES with base 0 - the host repeats with the multi-launch
// form, and nothing ever spins without bound.
template <typename T> __device__ __forceinline__ T look_back(T* __restrict__ chain, int chunk, T total, unsigned* __restrict__ stuck, unsigned stuckBit) {
    const int lane = threadIdx.x & 63;
    if (chunk == 0) {          // nothing in front: its own total is inclusive
        if (lane == 0) __hip_atomic_store(&chain[0], (T)((total << 2) | (T)2), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return (T)0;
    }
    if (lane == 0) __hip_atomic_store(&chain[chunk], (T)((total << 2) | (T)1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const long long t0 = wall_clock64();
    T base = 0;
    int hi = chunk - 1;                 // the nearest predecessor not yet accounted for
    for (;;) {
        const int idx = hi - lane;
        // (in front of chunk 0: nothing, inclusive)
        const T v = idx >= 0 ? __hip_atomic_load(&chain[idx], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : (T)2;
        const u64 ready = __ballot((v & (T)3) != (T)0), incl = __ballot((v & (T)3) == (T)2);
        T take = 0; bool done = false, moved = false;
        if (incl) {
            const int f = __ffsll((long long)incl) - 1;               // the nearest inclusive total
            const u64 below = (1ull << f) - 1ull;
            if ((ready & below) == below) { take = lane <= f ? v >> 2 : (T)0; done = true; }
        } else if (ready == ~0ull) { take = v >> 2; moved = true; }           // 64 own totals: add them, look further back
        if (done || moved) {
            base += wave_sum(take);
            if (done) break;
            hi -= 64;
            continue;
        }
        if (wall_clock64() - t0 > LOOK_BACK_TIMEOUT_TICKS) { if (lane == 0) atomicOr(stuck, stuckBit); base = 0; break; }
        __builtin_amdgcn_s_sleep(1);
    }
    if (lane == 0) __hip_atomic_store(&chain[chunk], (T)(((base + total) << 2) | (T)2), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return base;
}

}  // namespace rsq
