// mutate.h — kernels of the row mutations of a FLAT handle (mutate_host.inc): in-place row updates, the compaction that drops rows and
// the gather of rows by index.  The ROW MUTATION block of include/lynse_hip.h states the contract, DESIGN.md §22 the reasoning.
#pragma once
#include "common.h"

namespace lynse {

// k_scatter_rows: row rows[r] of the shard (pitch dst_pitch elements of T) <- dense f32 row r of src (width columns), pad columns zero.
// T = _Float16 rounds like k_f32_to_f16_rows (the one conversion, RNE): an updated row holds the bits an appended row would.  The rows
// are pairwise distinct (checked on the host), so no two items write one address.
template <typename T>
__global__ void __launch_bounds__(256) k_scatter_rows(T* __restrict__ dst, uint32_t dst_pitch, const uint64_t* __restrict__ rows,
                                                      const float* __restrict__ src, uint32_t width, uint64_t nrows) {
    const uint64_t total = nrows * dst_pitch;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t r = i / dst_pitch;
        const uint32_t c = (uint32_t)(i % dst_pitch);
        dst[rows[r] * dst_pitch + c] = c < width ? (T)src[r * width + c] : (T)0.0f;
    }
}

// k_gather_rows: dense f32 row r of dst (width columns) <- row rows[r] of the shard, any order, repeats allowed; T = _Float16 decodes
// exactly like k_f16_to_f32_rows.
template <typename T>
__global__ void __launch_bounds__(256) k_gather_rows(float* __restrict__ dst, const T* __restrict__ src, uint32_t src_pitch,
                                                     const uint64_t* __restrict__ rows, uint32_t width, uint64_t nrows) {
    const uint64_t total = nrows * width;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t r = i / width;
        const uint32_t c = (uint32_t)(i % width);
        dst[i] = (float)src[rows[r] * src_pitch + c];
    }
}

// k_compact_rows: one window of a compaction.  src = the window's first source row, nrows of `units` pieces of U each (uint4: 16 bytes,
// every pitch the library produces; uint32_t otherwise); keep / base = the window's first 64-row word of the keep bits (bits at or
// beyond the shard's length already cleared) and of the plan's exclusive prefix of their popcounts.  A kept row goes to row
//   base[w] + popcount(keep[w] & lower bits) - rank0
// of dst: dst = the shard's row rank0 (the direct path: the host has checked that the window's destinations end at or before its first
// source row, so no workgroup writes what another still has to read) or the dense scratch (the staged path).  The rank is a function of
// the plan alone: no atomics, no dependence on which wave gets anywhere first.  A copy kernel: one 16-byte piece per lane, consecutive
// lanes on consecutive pieces, two pieces in flight per lane; the (row, piece) pair advances by the grid's stride without a division.
template <typename U>
__global__ void __launch_bounds__(256) k_compact_rows(U* dst, const U* src, uint32_t units, const uint64_t* __restrict__ keep,
                                                      const uint32_t* __restrict__ base, uint32_t rank0, uint64_t nrows) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    const uint64_t dr = stride / units;
    const uint32_t dc = (uint32_t)(stride % units);
    const uint64_t i0 = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint64_t r = i0 / units;
    uint32_t c = (uint32_t)(i0 % units);
    auto step = [&](uint64_t& rr, uint32_t& cc) {
        rr += dr;
        cc += dc;
        if (cc >= units) { cc -= units; ++rr; }
    };
    auto target = [&](uint64_t rr, bool* kept) -> uint64_t {   // the destination row of source row rr (inside dst), and whether it stays
        const uint64_t w = keep[rr >> 6];
        const uint32_t b = (uint32_t)(rr & 63);
        *kept = (w >> b) & 1ull;
        return (uint64_t)base[rr >> 6] + (uint64_t)__popcll(w & ((1ull << b) - 1ull)) - rank0;
    };
    while (r < nrows) {
        uint64_t r2 = r;
        uint32_t c2 = c;
        step(r2, c2);
        bool k1 = false, k2 = false;
        const uint64_t t1 = target(r, &k1);
        const uint64_t t2 = r2 < nrows ? target(r2, &k2) : 0;
        U v1{}, v2{};
        if (k1) v1 = src[r * units + c];
        if (k2) v2 = src[r2 * units + c2];
        if (k1) dst[t1 * units + c] = v1;
        if (k2) dst[t2 * units + c2] = v2;
        r = r2;
        c = c2;
        step(r, c);
    }
}

}  // namespace lynse
