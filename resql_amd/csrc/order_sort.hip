// order_sort.hip — the rows of a materialisation ordered by their ORDER BY keys on the device, and their tuples delivered in that order
// (rsq_ctx_set_order_sort, rsq_prim_sort_rows, rsq_prim_gather_tuples).  The host's quicksort over all tuples (tail.cpp
// runMaterializeSort) stays the definition of the answer; the device's order - keys, then scan order - is the same wherever no two
// adjacent rows tie on all keys, which k_os_ties counts.  The image of a key cell and the layout of the composite key are
// order_sort.h's, which both sides use.
//   k_os_range           minimum and maximum image of every key column in one pass over the rows: per lane, wave reduction, LDS, then
//                        one 64-bit atomic min and max per workgroup and key
//   k_os_keys            keys[i] = one 64-bit word of the composite key of row perm[i] (the identity for the first word, which is
//                        written out too): the word's pieces gathered from the key columns
//                        -> radixSortPairs (devtail.hip) over (keys, perm), least significant word first: stable, so LSD over words
//   k_os_ties            the positions i, i + 1 < lead, whose rows perm[i] and perm[i + 1] have equal images on every key: a ballot,
//                        one atomic per wave that holds a tie
//   k_os_gather_tuples   out tuple i = in tuple perm[i]: a workgroup takes R = min(256, OS_TILE_BYTES / tuple size) consecutive
//                        output rows, whose span is staged in an LDS tile at its position inside a 16-byte group and stored 16
//                        bytes per lane between its ragged ends; the source tuples, at any byte address, are loaded as aligned 32-bit
//                        words where tuple size and addresses allow and as bytes otherwise; a tuple longer than the tile (R = 0) goes
//                        global to global, one lane per (row, 16-byte piece or byte)
// A row's byte offset is 64-bit (rows x tuple size passes 2^32); offsets inside the tile are 32-bit.
#include <algorithm>

#include "engine.h"
#include "order_sort.h"

namespace rsq {

typedef long long i64;
typedef unsigned long long u64;
typedef unsigned int u32;

#define OS_LANES 256
#define OS_TILE_BYTES 49152           /* LDS tile: the span of a workgroup's tuples, as k_pack_tuples' */
#define OS_TILE_SLACK 32              /* the span starts up to 15 bytes into the tile and is stored in whole 16-byte groups */
#define OS_PERM_BYTES (OS_LANES * 4)  /* the workgroup's rows of the permutation in front of the tile: a multiple of 16 */

namespace {

struct OsKey { const unsigned char* ptr; int32_t width, desc; };
struct OsKeys { int32_t n, pad; OsKey k[osort::MAX_KEYS]; };
// a piece of a word with all it takes to read it: the key column, its least image, and where the bits come from and go
struct OsPiece { const unsigned char* ptr; u64 min; int32_t width, desc, srcShift, dstShift, bits, pad; };
struct OsWord { int32_t nPieces, pad; OsPiece p[osort::MAX_KEYS]; };

// range[k]: least image of key k, range[MAX_KEYS + k]: greatest; preset to ~0 and 0
__global__ void __launch_bounds__(OS_LANES) k_os_range(OsKeys keys, i64 n, u64* __restrict__ range) {
    __shared__ u64 s_min[OS_LANES / 64][osort::MAX_KEYS], s_max[OS_LANES / 64][osort::MAX_KEYS];
    u64 mn[osort::MAX_KEYS], mx[osort::MAX_KEYS];
#pragma unroll
    for (int k = 0; k < osort::MAX_KEYS; k++) { mn[k] = ~0ull; mx[k] = 0ull; }
    for (i64 i = (i64)blockIdx.x * OS_LANES + threadIdx.x; i < n; i += (i64)gridDim.x * OS_LANES) {
#pragma unroll
        for (int k = 0; k < osort::MAX_KEYS; k++) {
            if (k < keys.n) {
                const u64 im = osort::image(keys.k[k].ptr + i * keys.k[k].width, keys.k[k].width, keys.k[k].desc != 0);
                mn[k] = im < mn[k] ? im : mn[k];
                mx[k] = im > mx[k] ? im : mx[k];
            }
        }
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < osort::MAX_KEYS; k++) {
        if (k < keys.n) {
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                const u64 a = __shfl_xor(mn[k], off), b = __shfl_xor(mx[k], off);
                mn[k] = a < mn[k] ? a : mn[k];
                mx[k] = b > mx[k] ? b : mx[k];
            }
            if (lane == 0) { s_min[wave][k] = mn[k]; s_max[wave][k] = mx[k]; }
        }
    }
    __syncthreads();
    if ((int)threadIdx.x < keys.n) {
        u64 a = s_min[0][threadIdx.x], b = s_max[0][threadIdx.x];
        for (int w = 1; w < OS_LANES / 64; w++) {
            a = s_min[w][threadIdx.x] < a ? s_min[w][threadIdx.x] : a;
            b = s_max[w][threadIdx.x] > b ? s_max[w][threadIdx.x] : b;
        }
        atomicMin(&range[threadIdx.x], a);
        atomicMax(&range[osort::MAX_KEYS + threadIdx.x], b);
    }
}

// permIn null: row i (and permOut[i] = i is written); else row permIn[i].  Every row number is below the rows of the key columns.
__global__ void __launch_bounds__(OS_LANES) k_os_keys(OsWord W, const u32* __restrict__ permIn, i64 n, u64* __restrict__ keysOut, u32* __restrict__ permOut) {
    for (i64 i = (i64)blockIdx.x * OS_LANES + threadIdx.x; i < n; i += (i64)gridDim.x * OS_LANES) {
        const i64 row = permIn ? (i64)permIn[i] : i;
        u64 v = 0;
#pragma unroll
        for (int p = 0; p < osort::MAX_KEYS; p++) {
            if (p < W.nPieces) {
                const u64 im = osort::image(W.p[p].ptr + row * W.p[p].width, W.p[p].width, W.p[p].desc != 0);
                v |= (((im - W.p[p].min) >> W.p[p].srcShift) & osort::lowMask(W.p[p].bits)) << W.p[p].dstShift;
            }
        }
        keysOut[i] = v;
        if (permOut) permOut[i] = (u32)i;
    }
}

// *count += the positions i with i + 1 < lead whose rows perm[i], perm[i + 1] are equal on every key
__global__ void __launch_bounds__(OS_LANES) k_os_ties(OsKeys keys, const u32* __restrict__ perm, i64 lead, u32* __restrict__ count) {
    for (i64 base = (i64)blockIdx.x * OS_LANES; base + 1 < lead; base += (i64)gridDim.x * OS_LANES) {      // (uniform in the workgroup: every lane reaches the ballot)
        const i64 i = base + threadIdx.x;
        bool tie = false;
        if (i + 1 < lead) {
            const i64 a = (i64)perm[i], b = (i64)perm[i + 1];
            tie = true;
#pragma unroll
            for (int k = 0; k < osort::MAX_KEYS; k++) {
                if (k < keys.n) {
                    const int w = keys.k[k].width;
                    tie = tie && osort::image(keys.k[k].ptr + a * w, w, keys.k[k].desc != 0) == osort::image(keys.k[k].ptr + b * w, w, keys.k[k].desc != 0);
                }
            }
        }
        const u64 m = __ballot(tie);
        if ((threadIdx.x & 63) == 0 && m) atomicAdd(count, (u32)__popcll(m));
    }
}

// mode 0: bytes; 1: aligned 32-bit words (ts, in and out are multiples of 4); 2 (R == 0 only): 16-byte pieces (ts, in and out are
// multiples of 16).  in: tuples of ts bytes, every perm[i] below their number; out: outRows tuples.  Dynamic LDS: OS_PERM_BYTES, and
// where R > 0 the tile of R x ts (rounded up to 16) + OS_TILE_SLACK bytes behind it.
__global__ void __launch_bounds__(OS_LANES) k_os_gather_tuples(const unsigned char* __restrict__ in, unsigned char* __restrict__ out, const u32* __restrict__ perm,
                                                                unsigned ts, i64 outRows, unsigned R, int mode) {
    extern __shared__ __attribute__((aligned(16))) unsigned char s_mem[];
    u32* s_perm = (u32*)s_mem;
    unsigned char* s_tile = s_mem + OS_PERM_BYTES;
    const unsigned tid = threadIdx.x;
    if (R == 0) {          // (uniform) one tuple is longer than the tile: global to global
        const i64 per = mode == 2 ? (i64)(ts / 16u) : (i64)ts;
        const i64 item = (i64)blockIdx.x * OS_LANES + tid;
        const i64 row = item / per;
        if (row >= outRows) return;
        const i64 k = item - row * per;
        const unsigned char* src = in + (i64)perm[row] * (i64)ts;
        unsigned char* dst = out + row * (i64)ts;
        if (mode == 2) ((uint4*)dst)[k] = ((const uint4*)src)[k];
        else dst[k] = src[k];
        return;
    }
    const i64 row0 = (i64)blockIdx.x * R;
    const unsigned nr = outRows - row0 < (i64)R ? (unsigned)(outRows - row0) : R;
    if (tid < nr) s_perm[tid] = perm[row0 + tid];
    __syncthreads();
    // the tuples' span: tile byte head + r * ts is output row row0 + r's first, and tile byte p is dst[p - head]
    unsigned char* dst = out + row0 * (i64)ts;
    const unsigned head = (unsigned)((uintptr_t)dst & 15u), spanEnd = head + nr * ts;
    if (mode == 1) {          // (head is a multiple of 4: out and ts are)
        const unsigned wpt = ts / 4u, total = nr * wpt;
        for (unsigned idx = tid; idx < total; idx += OS_LANES) {
            const unsigned r = idx / wpt, k = idx - r * wpt;
            *(u32*)(s_tile + head + r * ts + 4u * k) = ((const u32*)(in + (i64)s_perm[r] * (i64)ts))[k];
        }
    } else {
        const unsigned total = nr * ts;
        for (unsigned idx = tid; idx < total; idx += OS_LANES) {
            const unsigned r = idx / ts, k = idx - r * ts;
            s_tile[head + idx] = in[(i64)s_perm[r] * (i64)ts + k];
        }
    }
    __syncthreads();
    // the span out: its neighbours on either side are other workgroups', so whole 16-byte groups are stored only where all 16 bytes are
    // this workgroup's (as k_pack_tuples and k_text_write do)
    const unsigned a = head, b = spanEnd;
    const unsigned fullBegin = (a + 15u) & ~15u, fullEnd = b & ~15u;
    const unsigned headEnd = fullBegin < b ? fullBegin : b;
    const unsigned tailBegin = fullEnd > headEnd ? fullEnd : headEnd;
    for (unsigned p = fullBegin + tid * 16u; p < fullEnd; p += OS_LANES * 16u) *(uint4*)(dst + (p - a)) = *(const uint4*)(s_tile + p);
    if (tid < headEnd - a) dst[tid] = s_tile[a + tid];
    if (tid >= 64u && tid - 64u < b - tailBegin) dst[tailBegin - a + (tid - 64u)] = s_tile[tailBegin + (tid - 64u)];
}

unsigned gridFor(Context& ctx, int64_t n) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>(8 * (int64_t)ctx.numCUs, (n + OS_LANES - 1) / OS_LANES)); }

// output rows a workgroup of k_os_gather_tuples stages in LDS (0: a tuple is longer than the tile)
int gatherGroupRows(int tupleSize) { return tupleSize <= OS_TILE_BYTES ? (int)std::min<int64_t>(OS_LANES, OS_TILE_BYTES / tupleSize) : 0; }

}  // namespace

void OrderSortBuffers::ensure(Context& ctx, int64_t nRows) {
    if (!dStatus) dStatus = (uint64_t*)ctx.alloc(256);
    if (!hStatus) hStatus = (uint64_t*)ctx.allocPinned(256);
    for (hipEvent_t& e : ev) if (!e) e = ctx.takeEvent();
    if (dKeys[0] && nRows <= rows) return;
    for (int s = 0; s < 2; s++) {
        if (dKeys[s]) ctx.free(dKeys[s]);
        if (dPerm[s]) ctx.free(dPerm[s]);
        dKeys[s] = nullptr; dPerm[s] = nullptr;
    }
    if (dTemp) ctx.free(dTemp);
    dTemp = nullptr; rows = 0;
    const size_t n = (size_t)std::max<int64_t>(nRows, 2);
    for (int s = 0; s < 2; s++) { dKeys[s] = (uint64_t*)ctx.alloc(n * 8); dPerm[s] = (uint32_t*)ctx.alloc(n * 4); }
    tempBytes = radixSortTempBytes((int64_t)n);
    dTemp = ctx.alloc(tempBytes);
    rows = (int64_t)n;
}

void OrderSortBuffers::release(Context& ctx) {
    for (int s = 0; s < 2; s++) {
        if (dKeys[s]) ctx.free(dKeys[s]);
        if (dPerm[s]) ctx.free(dPerm[s]);
    }
    if (dTemp) ctx.free(dTemp);
    if (dStatus) ctx.free(dStatus);
    if (hStatus) ctx.freePinned(hStatus);
    for (hipEvent_t e : ev) ctx.giveEvent(e);
    *this = OrderSortBuffers();
}

void orderSortRows(Context& ctx, OrderSortBuffers& b, const OrderSortKey* keys, int nKeys, int64_t nRows, int64_t lead, OrderSortOutcome& out) {
    if (nKeys < 1 || nKeys > (int)osort::MAX_KEYS || nRows < 1 || nRows >= ((int64_t)1 << 32) || lead < 0 || lead > nRows || !b.dKeys[0] || b.rows < nRows)
        throw Error(RSQ_ERR_RUNTIME, "internal error: order_sort outside its buffers");
    OsKeys ks{};
    ks.n = nKeys;
    for (int k = 0; k < nKeys; k++) {
        if (keys[k].width != 4 && keys[k].width != 8) throw Error(RSQ_ERR_RUNTIME, "internal error: order_sort met a key of " + std::to_string(keys[k].width) + " bytes");
        ks.k[k].ptr = (const unsigned char*)keys[k].ptr; ks.k[k].width = keys[k].width; ks.k[k].desc = keys[k].desc ? 1 : 0;
    }
    out = OrderSortOutcome();
    u64* dRange = (u64*)b.dStatus;
    u32* dTies = (u32*)(b.dStatus + 2 * osort::MAX_KEYS);
    RSQ_HIP(hipEventRecord(b.ev[0], ctx.stream));
    RSQ_HIP(hipMemsetAsync(dRange, 0xff, osort::MAX_KEYS * 8, ctx.stream));
    RSQ_HIP(hipMemsetAsync(dRange + osort::MAX_KEYS, 0, osort::MAX_KEYS * 8 + 8, ctx.stream));          // (the greatest images and the tie count)
    hipLaunchKernelGGL(k_os_range, dim3(gridFor(ctx, nRows)), dim3(OS_LANES), 0, ctx.stream, ks, (i64)nRows, dRange);
    RSQ_HIP(hipGetLastError());
    RSQ_HIP(hipEventRecord(b.ev[1], ctx.stream));
    out.launches = 1;
    RSQ_HIP(hipMemcpyAsync(b.hStatus, dRange, 2 * osort::MAX_KEYS * 8, hipMemcpyDeviceToHost, ctx.stream));
    RSQ_HIP(hipStreamSynchronize(ctx.stream));          // the first of the two waits: the layout decides the passes
    ctx.streamDrained();
    const osort::Layout L = osort::layoutOf(b.hStatus, b.hStatus + osort::MAX_KEYS, nKeys);
    for (int k = 0; k < nKeys; k++) out.bits[k] = L.bits[k];
    out.totalBits = L.totalBits; out.words = L.nWords; out.passes = osort::passesOf(L);
    RSQ_HIP(hipEventRecord(b.ev[2], ctx.stream));
    if (L.totalBits == 0 && lead > 1) {          // every row equals every other on all keys: nothing to sort, and the answer is the host's
        out.sorted = false;
        out.tiedPairs = lead - 1;
        RSQ_HIP(hipEventRecord(b.ev[3], ctx.stream));
        return;
    }
    int cur = 0;          // which side holds the permutation
    for (int w = 0; w < std::max(L.nWords, 1); w++) {
        OsWord W{};
        W.nPieces = L.word[w].nPieces;
        for (int p = 0; p < W.nPieces; p++) {
            const osort::Piece& pc = L.word[w].piece[p];
            W.p[p].ptr = ks.k[pc.key].ptr; W.p[p].min = L.min[pc.key]; W.p[p].width = ks.k[pc.key].width; W.p[p].desc = ks.k[pc.key].desc;
            W.p[p].srcShift = pc.srcShift; W.p[p].dstShift = pc.dstShift; W.p[p].bits = pc.bits;
        }
        hipLaunchKernelGGL(k_os_keys, dim3(gridFor(ctx, nRows)), dim3(OS_LANES), 0, ctx.stream, W, w == 0 ? (const u32*)nullptr : (const u32*)b.dPerm[cur], (i64)nRows,
                           (u64*)b.dKeys[cur], w == 0 ? (u32*)b.dPerm[cur] : (u32*)nullptr);
        RSQ_HIP(hipGetLastError());
        out.launches += 1;
        const int bits = L.word[w].bits;
        const bool moved = radixSortPairs(ctx, b.dKeys[cur], b.dPerm[cur], b.dKeys[cur ^ 1], b.dPerm[cur ^ 1], nRows, bits, b.dTemp, b.tempBytes);
        if (nRows > 1 && bits > 0) out.launches += 5 * ((bits + 7) / 8);          // a pass: histogram, three kernels of the scan, scatter
        if (moved) cur ^= 1;
    }
    out.dPerm = b.dPerm[cur];
    if (lead > 1) {
        hipLaunchKernelGGL(k_os_ties, dim3(gridFor(ctx, lead)), dim3(OS_LANES), 0, ctx.stream, ks, (const u32*)out.dPerm, (i64)lead, dTies);
        RSQ_HIP(hipGetLastError());
        out.launches += 1;
    }
    out.dTies = dTies;
    RSQ_HIP(hipEventRecord(b.ev[3], ctx.stream));
}

void gatherTuples(Context& ctx, const uint8_t* dIn, uint8_t* dOut, const uint32_t* dPerm, int tupleSize, int64_t outRows) {
    if (tupleSize < 1 || outRows < 0 || outRows >= ((int64_t)1 << 32)) throw Error(RSQ_ERR_RUNTIME, "internal error: gatherTuples outside its range");
    if (outRows == 0) return;
    const int R = gatherGroupRows(tupleSize);
    const uintptr_t addr = (uintptr_t)dIn | (uintptr_t)dOut | (uintptr_t)tupleSize;
    const int mode = R ? ((addr & 3u) == 0 ? 1 : 0) : ((addr & 15u) == 0 ? 2 : 0);
    const int64_t per = mode == 2 ? tupleSize / 16 : tupleSize;
    const int64_t groups = R ? (outRows + R - 1) / R : (outRows * per + OS_LANES - 1) / OS_LANES;
    if (groups > 0x7fffffffll) failInvalid("gatherTuples: more workgroups than a launch takes");
    const size_t lds = OS_PERM_BYTES + (R ? (((size_t)R * (size_t)tupleSize + 15) & ~(size_t)15) + OS_TILE_SLACK : 0);
    hipLaunchKernelGGL(k_os_gather_tuples, dim3((unsigned)groups), dim3(OS_LANES), lds, ctx.stream, (const unsigned char*)dIn, (unsigned char*)dOut, (const u32*)dPerm,
                       (unsigned)tupleSize, (i64)outRows, (unsigned)R, mode);
    RSQ_HIP(hipGetLastError());
}

}  // namespace rsq
