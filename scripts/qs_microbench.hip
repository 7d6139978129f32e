// qs_microbench.hip — stand-alone A/B of the int8 scan kernels on synthetic codes (development tool, not product):
//   k_scan_h16<2,4,4,2,IP,…,I8Q=2>  (256 x 256 tile, query image through the LDS-DMA ring)   vs
//   k_scan_qs<…>                     (query-stationary: B operand in registers, rows-only LDS ring; scan_qs.h)
// 1. correctness: both kernels over a small shard (ragged last tile) against a brute-force kernel — identical key sets;
// 2. timing: interleaved rounds over a large shard, HIP events, plus the shader clock each QS variant held
//    (s_memtime ticks of workgroup 0 / event time) and wall-clock stamps a power sampler can be joined on.
// 0. `qs_microbench operand [rows rounds sigma]`: the operand-distribution axis instead (row bytes uniform / non-negative / 6-bit / constant x
//    query image non-negative / mixed sign, the library's default instantiation with and without emission; profiles/sq7_operand_energy.txt).
// 1b. `qs_microbench qs16 [rows rounds sigma]`: the MFMA-shape axis: the default instantiation against its 16x16x64 form (scan_qs.h, M16) — the check
//    passes of both, then everything / MFMA only / MFMA + LDS reads / DMA + MFMA of both in interleaved rounds, on SQ7-like and centred operands, with
//    the s_memtime clock, the socket power and the cycles per MFMA (profiles/qs16_microbench.txt).
// Build: hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -mllvm -pragma-unroll-threshold=262144 \
//        [-DLYNSE_EXPERIMENTS] -o qs_microbench scripts/qs_microbench.hip
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <atomic>
#include <dirent.h>
#include <fstream>
#include <functional>
#include <string>
#include <thread>
#include <type_traits>
#include <utility>
#include <vector>

#include "../lynsedb_amd/csrc/kernels.h"
#include "../lynsedb_amd/csrc/scan_qs.h"
#include "scan_qs2.h"   // (the measured-negative one-wave-per-SIMD form: kept beside this microbenchmark, not in the product directory)

using namespace lynse;

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s:%d %s: %s\n", __FILE__, __LINE__, #x, hipGetErrorString(e_)); exit(1); } } while (0)

__device__ __host__ inline uint32_t mix(uint64_t x) {
    x ^= x >> 33; x *= 0xff51afd7ed558ccdull; x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ull; x ^= x >> 33;
    return (uint32_t)x;
}
// (and_mask, or_bits) shape the byte distribution: 0xffffffff / 0 = uniform int8, 0x7f7f7f7f = [0,127], 0x3f3f3f3f = [0,63], 0 / c c c c = constant
__global__ void k_fill_rows(int8_t* V, uint64_t nbytes, uint64_t seed, uint32_t and_mask = 0xffffffffu, uint32_t or_bits = 0u) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i * 4 < nbytes; i += (uint64_t)gridDim.x * blockDim.x)
        reinterpret_cast<uint32_t*>(V)[i] = (mix(i + seed * 0x9e3779b97f4a7c15ull) & and_mask) | or_bits;
}
// queries: plain [nq][D] int8 in [-127,127] (nonneg: [0,127]) and the kernel's image [nslab][qpad][8 slots ^ swizzle][16]
__device__ __host__ inline int query_elem(uint32_t q, uint32_t i, bool nonneg) {
    const uint32_t h = mix(0x1234567ull + (uint64_t)q * 100003 + i);
    return nonneg ? (int)(h % 128u) : (int)(h % 255u) - 127;
}
__global__ void k_fill_queries(int8_t* plain, int8_t* img, uint32_t nq, uint32_t qpad, uint32_t D, uint32_t nslab, bool nonneg = false) {
    const uint32_t q = blockIdx.x;
    for (uint32_t i = threadIdx.x; i < nslab * 128; i += blockDim.x) {
        int u = 0;
        if (q < nq && i < D) { u = query_elem(q, i, nonneg); plain[(size_t)q * D + i] = (int8_t)u; }
        const uint32_t s = i / 128, k = i % 128, l = k >> 4, e = k & 15, p = l ^ ((q >> 1) & 7);
        img[(((size_t)s * qpad + q) * 8 + p) * 16 + e] = (int8_t)u;
    }
}
// brute force: one workgroup per row block of 64 rows, thread = (row, query stripe)
__global__ void __launch_bounds__(256) k_ref(const int8_t* V, uint32_t ld, uint32_t D, uint32_t n, const int8_t* Qp, uint32_t nq,
                                             const int* T, uint64_t* out, uint32_t* out_n, uint32_t out_cap,
                                             const float* vn2 = nullptr, const float* sq = nullptr, const float* bq = nullptr, const float* thr = nullptr) {
    const uint32_t row = blockIdx.x * 64 + (threadIdx.x & 63);
    if (row >= n) return;
    for (uint32_t q = threadIdx.x >> 6; q < nq; q += 4) {
        int dot = 0;
        for (uint32_t d = 0; d < D; ++d) dot += (int)V[(size_t)row * ld + d] * (int)Qp[(size_t)q * D + d];
        if (vn2) {   // squared L2 on the plain codes: |v|^2 - 2 s_q dot + c_q <= thr (separate mul / add like the kernels)
            float sc = (float)dot * sq[q];
            sc = vn2[row] - 2.0f * sc + bq[q];
            if (sc <= thr[q]) {
                const uint32_t slot = atomicAdd(out_n, 1u);
                if (slot < out_cap) out[slot] = ((uint64_t)q << 48) ^ make_key(sc, row, true);
            }
            continue;
        }
        if (dot >= T[q]) {
            const uint32_t slot = atomicAdd(out_n, 1u);
            if (slot < out_cap) out[slot] = ((uint64_t)q << 48) ^ make_key((float)dot, row, false);
        }
    }
}

// amdgpu hwmon: socket power (uW) and shader clock (Hz), sampled by a background thread while a variant runs
struct Sampler {
    std::string power_path, freq_path;
    std::atomic<bool> on{false}, stop{false};
    std::atomic<long long> sum_p{0}, sum_f{0}, n{0};
    std::thread th;
    static bool read_ll(const std::string& p, long long* v) { std::ifstream f(p); return (bool)(f >> *v); }
    void start() {
        char bus[64] = {0};
        if (hipDeviceGetPCIBusId(bus, sizeof(bus), 0) == hipSuccess) {
            for (char* c = bus; *c; ++c) *c = (char)tolower(*c);
            const std::string hw = std::string("/sys/bus/pci/devices/") + bus + "/hwmon";
            if (DIR* d = opendir(hw.c_str())) {
                while (dirent* e = readdir(d)) {
                    if (e->d_name[0] == '.') continue;
                    const std::string base = hw + "/" + e->d_name;
                    long long v;
                    for (const char* pn : {"/power1_average", "/power1_input"})
                        if (power_path.empty() && read_ll(base + pn, &v)) power_path = base + pn;
                    if (freq_path.empty() && read_ll(base + "/freq1_input", &v)) freq_path = base + "/freq1_input";
                }
                closedir(d);
            }
            printf("device pci %s\n", bus);
        }
        DIR* d = power_path.empty() ? opendir("/sys/class/hwmon") : nullptr;
        if (d) {
            while (dirent* e = readdir(d)) {
                const std::string base = std::string("/sys/class/hwmon/") + e->d_name;
                std::ifstream nf(base + "/name");
                std::string name;
                if (!(nf >> name) || name != "amdgpu") continue;
                long long v;
                for (const char* pn : {"/power1_average", "/power1_input"})
                    if (power_path.empty() && read_ll(base + pn, &v)) power_path = base + pn;
                if (freq_path.empty() && read_ll(base + "/freq1_input", &v)) freq_path = base + "/freq1_input";
            }
            closedir(d);
        }
        printf("sampler: power %s, sclk %s\n", power_path.c_str(), freq_path.c_str());
        th = std::thread([this]() {
            while (!stop.load()) {
                if (on.load()) {
                    long long p = 0, f = 0;
                    if (!power_path.empty()) read_ll(power_path, &p);
                    if (!freq_path.empty()) read_ll(freq_path, &f);
                    sum_p += p; sum_f += f; n += 1;
                }
                std::this_thread::sleep_for(std::chrono::milliseconds(2));
            }
        });
    }
    void begin() { sum_p = 0; sum_f = 0; n = 0; on = true; }
    void end(double* watts, double* mhz) { on = false; const double k = (double)std::max<long long>(n.load(), 1); *watts = sum_p / k * 1e-6; *mhz = sum_f / k * 1e-6; }
    void finish() { stop = true; if (th.joinable()) th.join(); }
};

// every dot product of a small shard (STS check)
__global__ void __launch_bounds__(256) k_all_dots(const int8_t* V, uint32_t ld, uint32_t D, uint32_t n, const int8_t* Qp, uint32_t nq, int* out) {
    const uint32_t row = blockIdx.x * 64 + (threadIdx.x & 63);
    if (row >= n) return;
    for (uint32_t q = threadIdx.x >> 6; q < nq; q += 4) {
        int dot = 0;
        for (uint32_t d = 0; d < D; ++d) dot += (int)V[(size_t)row * ld + d] * (int)Qp[(size_t)q * D + d];
        out[(size_t)q * n + row] = dot;
    }
}
// stand-in for the seeding of k_i8c_prep_queries: partition maxima over a few sample rows
__global__ void __launch_bounds__(256) k_seed(const int8_t* V, uint32_t ld, uint32_t D, uint32_t n, const int8_t* Qp, uint32_t rt, uint32_t ks,
                                              uint32_t seed_rows, int* dyn_thr, int* dyn_slot, int* dyn_marg, int marg) {
    __shared__ int s_slot[32];
    const uint32_t q = blockIdx.x, tid = threadIdx.x;
    if (tid < 32) s_slot[tid] = -2147483647 - 1;
    __syncthreads();
    const uint32_t ntiles = (n + rt - 1) / rt, per = seed_rows / ks;
    for (uint32_t i = tid; i < per * ks; i += 256) {
        const uint32_t p = i % ks, m = i / ks;
        const uint32_t up = (ntiles > p) ? (ntiles - p + ks - 1) / ks : 0u;
        if (!up) continue;
        const uint32_t u_idx = (uint32_t)(((uint64_t)m * up) / per);
        uint64_t row = (uint64_t)(p + ks * u_idx) * rt + (i * 7u) % rt;
        if (row >= n) row = (uint64_t)(p + ks * u_idx) * rt;
        int dot = 0;
        for (uint32_t d = 0; d < D; ++d) dot += (int)V[row * ld + d] * (int)Qp[(size_t)q * D + d];
        atomicMax(&s_slot[p], dot);
    }
    __syncthreads();
    if (tid < 32) dyn_slot[(size_t)q * 32 + tid] = tid < ks ? s_slot[tid] : 2147483647;
    if (tid == 0) {
        int mn = 2147483647;
        for (uint32_t j = 0; j < ks; ++j) mn = s_slot[j] < mn ? s_slot[j] : mn;
        dyn_thr[q] = mn;
        dyn_marg[q] = marg;
    }
}

struct Bufs {
    int8_t *V = nullptr, *Qp = nullptr, *img = nullptr;
    float *qinv = nullptr, *qn2 = nullptr, *thr = nullptr;
    int* Ti = nullptr;
    uint64_t *cand = nullptr, *candB = nullptr;
    uint8_t* segcnt = nullptr;
    uint32_t* count = nullptr;
    unsigned long long* dbg = nullptr;
    int *dyn_thr = nullptr, *dyn_slot = nullptr, *dyn_marg = nullptr;
    float* vn2 = nullptr;
    uint32_t cap = 16384;
};

static const uint32_t D = 768, NSLABS = 6, NQ = 256, QPAD = 256;
static const uint32_t SEG_KEYS = 32768;

static ScanArgs base_args(const Bufs& b, uint32_t r0, uint32_t r1, uint32_t nq) {
    ScanArgs a{};
    a.V16 = reinterpret_cast<const _Float16*>(b.V); a.ld16 = D; a.D = D; a.ld = D;
    a.row0 = r0; a.row1 = r1; a.Q16 = reinterpret_cast<const _Float16*>(b.img);
    a.qpad = QPAD; a.nq = nq; a.nslab = NSLABS;
    a.qinv = b.qinv; a.qn2 = b.qn2; a.qrinv = b.qinv; a.thr = b.thr;
    a.cand = b.cand; a.count = b.count; a.cap = b.cap; a.candB = b.candB; a.segcnt = b.segcnt;
    a.emit_all = 0;
    a.vn2 = b.vn2; a.vrinv = b.vn2; a.vmax2 = 400.0f;
    a.dyn_thr = b.dyn_thr; a.dyn_slot = b.dyn_slot; a.dyn_marg = b.dyn_marg; a.dyn_ks = 10; a.dyn_warm = 4;
    return a;
}

template <typename K>
static void set_lds(K k, size_t bytes) { CK(hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes)); }

struct Variant {
    std::string name;
    int segs_per_wg;
    void (*launch)(ScanArgs a, uint32_t grid, hipStream_t st);
    bool qs;
};

template <int NSLAB, int RB, int SL, int NS, bool XPF, int NBUF, int DBG, int PP = 0, int STS = 0, int MET = 0, int M16 = 0>
static void launch_qs(ScanArgs a, uint32_t grid, hipStream_t st) {
    auto k = k_scan_qs<NSLAB, RB, SL, NS, XPF, NBUF, DBG, PP, STS, MET, 0, 0, 0, M16>;
    constexpr size_t lds = (size_t)NS * SL * RB * 32 * 128 + (STS ? QS_STS_LDS : 0) + (MET == 1 ? (NS + 1) * RB * 32 * 4 : 0);
    static bool done = false;
    if (!done) { set_lds(k, lds); done = true; }
    const uint32_t nt = (a.row1 - a.row0 + RB * 32 - 1) / (RB * 32);
    uint32_t g = std::min(grid, nt);
    if (STS) {   // contiguous chunks of `pitch` tiles per workgroup, pitch coprime to the partition count
        auto gcd = [](uint32_t x, uint32_t y) { while (y) { const uint32_t t = x % y; x = y; y = t; } return x; };
        uint32_t pitch = (nt + g - 1) / g;
        while (gcd(pitch, a.dyn_ks) != 1) ++pitch;
        a.dyn_pitch = pitch;
        g = (nt + pitch - 1) / pitch;
    }
    hipLaunchKernelGGL(k, dim3(g), dim3(512), lds, st, a);
}
// one wave per SIMD, two 32-query blocks per wave (scan_qs2.h)
template <int NSLAB, int RB, int NS, int NBUF, int DBG>
static void launch_qs2(ScanArgs a, uint32_t grid, hipStream_t st) {
    auto k = k_scan_qs2<NSLAB, RB, NS, NBUF, DBG>;
    constexpr size_t lds = (size_t)NS * NSLAB * RB * 32 * 128;
    static bool done = false;
    if (!done) { set_lds(k, lds); done = true; }
    const uint32_t nt = (a.row1 - a.row0 + RB * 32 - 1) / (RB * 32);
    hipLaunchKernelGGL(k, dim3(std::min(grid, nt)), dim3(256), lds, st, a);
}
// the round-3 squared-L2 kernel on the plain codes (<4,2,2,4> tiling, DENSE float epilogue, norm ring)
static void launch_old_l2(ScanArgs a, uint32_t grid, hipStream_t st) {
    auto k = k_scan_h16<4, 2, 2, 4, M_L2, 2, 2, 2, false, false, 0, false, 4, 0, true>;
    constexpr size_t lds = (size_t)(2 * 256 + 2 * 256) * 128 + 4 * 1024;
    static bool done = false;
    if (!done) { set_lds(k, lds); done = true; }
    a.ntiles = (a.row1 - a.row0 + 255) / 256;
    a.dense = 1;
    hipLaunchKernelGGL(k, dim3(std::min(grid, a.ntiles)), dim3(512), lds, st, a);
}
template <bool DENSE, int DBG>
static void launch_old(ScanArgs a, uint32_t grid, hipStream_t st) {
    auto k = k_scan_h16<2, 4, 4, 2, M_IP, 3, 2, 2, false, false, DBG, false, 2, 0, DENSE>;
    constexpr size_t lds = (size_t)(3 * 256 + 2 * 256) * 128;
    static bool done = false;
    if (!done) { set_lds(k, lds); done = true; }
    a.ntiles = (a.row1 - a.row0 + 255) / 256;
    a.dense = DENSE ? 1 : 0;
    hipLaunchKernelGGL(k, dim3(std::min(grid, a.ntiles)), dim3(512), lds, st, a);
}

static std::vector<std::vector<uint64_t>> collect_q(const Bufs& b, uint32_t nq, uint32_t nseg, uint32_t seg) {   // keys per query
    std::vector<uint32_t> cnt(nq);
    CK(hipMemcpy(cnt.data(), b.count, nq * 4, hipMemcpyDeviceToHost));
    std::vector<std::vector<uint64_t>> out(nq);
    std::vector<uint64_t> tmp(b.cap);
    for (uint32_t q = 0; q < nq; ++q) {
        const uint32_t c = std::min(cnt[q], b.cap);
        if (cnt[q] > b.cap) { fprintf(stderr, "query %u overflowed the shared region (%u)\n", q, cnt[q]); }
        if (c) {
            CK(hipMemcpy(tmp.data(), b.cand + (size_t)q * b.cap, (size_t)c * 8, hipMemcpyDeviceToHost));
            out[q].assign(tmp.begin(), tmp.begin() + c);
        }
    }
    if (nseg) {
        std::vector<uint8_t> sc((size_t)nq * nseg);
        std::vector<uint64_t> sk((size_t)nq * nseg * seg);
        CK(hipMemcpy(sc.data(), b.segcnt, sc.size(), hipMemcpyDeviceToHost));
        CK(hipMemcpy(sk.data(), b.candB, sk.size() * 8, hipMemcpyDeviceToHost));
        for (uint32_t q = 0; q < nq; ++q)
            for (uint32_t s = 0; s < nseg; ++s)
                for (uint32_t i = 0; i < sc[(size_t)q * nseg + s]; ++i) out[q].push_back(sk[((size_t)q * nseg + s) * seg + i]);
    }
    return out;
}
static std::vector<uint64_t> collect(const Bufs& b, uint32_t nq, uint32_t nseg, uint32_t seg) {
    std::vector<uint64_t> keys;
    const auto per = collect_q(b, nq, nseg, seg);
    for (uint32_t q = 0; q < nq; ++q)
        for (uint64_t k : per[q]) keys.push_back(((uint64_t)q << 48) ^ k);
    std::sort(keys.begin(), keys.end());
    return keys;
}

int main(int argc, char** argv) {
    // "operand" as the first argument: the operand-distribution axis (section 0 below) instead of the variant A/B; the other arguments follow it
    const bool operand_axis = argc > 1 && strcmp(argv[1], "operand") == 0;
    if (operand_axis) { --argc; ++argv; }
    // "qs16" as the first argument: the MFMA-shape A/B (section 1b below): the check passes of the default instantiation and of its 16x16x64
    // form only, then both forms and their decompositions timed in interleaved rounds on SQ7-like and on centred operands
    const bool qs16_axis = !operand_axis && argc > 1 && strcmp(argv[1], "qs16") == 0;
    if (qs16_axis) { --argc; ++argv; }
    const uint64_t n_big = argc > 1 ? strtoull(argv[1], nullptr, 10) : 10000000ull;
    const int rounds = argc > 2 ? atoi(argv[2]) : 5;
    const double sigma_tight = argc > 3 ? atof(argv[3]) : 4.3;   // thresholds in units of the dot product's standard deviation
    const int only = argc > 4 ? atoi(argv[4]) : -1;
    const double sigma_loose = argc > 7 ? atof(argv[7]) : 3.6;
    const double sts_marg_sd = argc > 8 ? atof(argv[8]) : 0.45;   // STS margin in units of the dot product's sd (bench data: 2E ~ 0.5 sd)
    const int long_reps = argc > 5 ? atoi(argv[5]) : 20, long_warm = argc > 6 ? atoi(argv[6]) : 25;
    Sampler sampler;
    sampler.start();
    hipDeviceProp_t prop;
    CK(hipGetDeviceProperties(&prop, 0));
    const uint32_t ncu = (uint32_t)prop.multiProcessorCount;
    printf("device %s, %u CUs\n", prop.name, ncu);
    Bufs b;
    CK(hipMalloc(&b.V, n_big * D + 4096));
    CK(hipMalloc(&b.Qp, (size_t)NQ * D));
    CK(hipMalloc(&b.img, (size_t)NSLABS * QPAD * 128));
    CK(hipMalloc(&b.qinv, NQ * 4)); CK(hipMalloc(&b.qn2, NQ * 4)); CK(hipMalloc(&b.thr, NQ * 4)); CK(hipMalloc(&b.Ti, NQ * 4));
    CK(hipMalloc(&b.cand, (size_t)NQ * b.cap * 8));
    CK(hipMalloc(&b.candB, (size_t)NQ * SEG_KEYS * 8));
    CK(hipMalloc(&b.segcnt, (size_t)NQ * 4096));
    CK(hipMalloc(&b.count, NQ * 4));
    CK(hipMalloc(&b.vn2, (n_big + 4096) * 4));
    {
        std::vector<float> hv(n_big + 4096);
        for (size_t i = 0; i < hv.size(); ++i) hv[i] = 200.0f + (float)(mix(i * 77 + 5) % 100000) * 1e-3f;
        CK(hipMemcpy(b.vn2, hv.data(), hv.size() * 4, hipMemcpyHostToDevice));
    }
    CK(hipMalloc(&b.dyn_thr, NQ * 4)); CK(hipMalloc(&b.dyn_marg, NQ * 4)); CK(hipMalloc(&b.dyn_slot, NQ * 32 * 4));
    CK(hipMalloc(&b.dbg, 4096 * 16));
    CK(hipMemset(b.dbg, 0, 4096 * 16));
    hipLaunchKernelGGL(k_fill_rows, dim3(ncu * 8), dim3(256), 0, 0, b.V, n_big * D, 7ull);
    CK(hipMemset(b.img, 0, (size_t)NSLABS * QPAD * 128));
    hipLaunchKernelGGL(k_fill_queries, dim3(QPAD), dim3(256), 0, 0, b.Qp, b.img, NQ, QPAD, D, NSLABS);
    CK(hipDeviceSynchronize());
    // dot product of a uniform byte in [-128,127] with a uniform byte in [-127,127]: sd = 73.9 * 73.3 per term
    const double sd = std::sqrt((double)D) * 73.9 * 73.3;
    auto set_thr_l2 = [&](double sig, uint32_t nq) {
        std::vector<float> sq(NQ, 1.0e-3f), bq(NQ), th(NQ);
        for (uint32_t q = 0; q < NQ; ++q) { bq[q] = 10.0f + (float)(q % 5); th[q] = q < nq ? (float)(200.0 + bq[q] - 2.0e-3 * sig * sd + 0.01 * (q % 7)) : -1e30f; }
        CK(hipMemcpy(b.qinv, sq.data(), NQ * 4, hipMemcpyHostToDevice));
        CK(hipMemcpy(b.qn2, bq.data(), NQ * 4, hipMemcpyHostToDevice));
        CK(hipMemcpy(b.thr, th.data(), NQ * 4, hipMemcpyHostToDevice));
    };
    auto set_thr = [&](double sig, uint32_t nq) {
        std::vector<float> one(NQ, 1.0f), zero(NQ, 0.0f), th(NQ);
        std::vector<int> ti(NQ);
        for (uint32_t q = 0; q < NQ; ++q) { th[q] = (float)std::floor(sig * sd + 1000.0 * (q % 7)); ti[q] = q < nq ? (int)th[q] : 0x7fffffff; }
        CK(hipMemcpy(b.qinv, one.data(), NQ * 4, hipMemcpyHostToDevice));
        CK(hipMemcpy(b.qn2, zero.data(), NQ * 4, hipMemcpyHostToDevice));
        CK(hipMemcpy(b.thr, th.data(), NQ * 4, hipMemcpyHostToDevice));
        CK(hipMemcpy(b.Ti, ti.data(), NQ * 4, hipMemcpyHostToDevice));
    };

    std::vector<Variant> vars;
    vars.push_back({"old<2,4,4,2> two-level", 4, launch_old<false, 0>, false});
    vars.push_back({"old<2,4,4,2> DENSE", 8, launch_old<true, 0>, false});
    vars.push_back({"qs RB1 SL6 NS6 XPF NBUF8", 2, launch_qs<6, 1, 6, 6, true, 8, 0>, true});
    vars.push_back({"qs RB2 SL3 NS6 XPF NBUF8", 2, launch_qs<6, 2, 3, 6, true, 8, 0>, true});
    vars.push_back({"qs RB2 SL6 NS3 noXPF NBUF8", 2, launch_qs<6, 2, 6, 3, false, 8, 0>, true});
    vars.push_back({"qs RB2 SL6 NS3 noXPF NBUF8 STS", 2, launch_qs<6, 2, 6, 3, false, 8, 0, 0, 1>, true});
    vars.push_back({"qs RB2 SL6 NS3 noXPF NBUF8 PP1 STS", 2, launch_qs<6, 2, 6, 3, false, 8, 0, 1, 1>, true});
    vars.push_back({"L2 old<4,2,2,4> DENSE", 4, launch_old_l2, false});
    vars.push_back({"L2 qs RB2 SL6 NS3 noXPF NBUF8 PP1", 2, launch_qs<6, 2, 6, 3, false, 8, 0, 1, 0, 1>, true});
    vars.push_back({"L2 qs RB2 SL6 NS3 noXPF NBUF8", 2, launch_qs<6, 2, 6, 3, false, 8, 0, 0, 0, 1>, true});
    vars.push_back({"qs RB1 SL6 NS6 XPF NBUF8 PP1", 2, launch_qs<6, 1, 6, 6, true, 8, 0, 1>, true});
    vars.push_back({"qs RB1 SL6 NS6 XPF NBUF8 PP2", 2, launch_qs<6, 1, 6, 6, true, 8, 0, 2>, true});
    vars.push_back({"qs RB1 SL6 NS6 XPF NBUF12 PP1", 2, launch_qs<6, 1, 6, 6, true, 12, 0, 1>, true});
    vars.push_back({"qs RB1 SL6 NS5 XPF NBUF8 PP1", 2, launch_qs<6, 1, 6, 5, true, 8, 0, 1>, true});
    vars.push_back({"qs RB2 SL6 NS3 noXPF NBUF8 PP1", 2, launch_qs<6, 2, 6, 3, false, 8, 0, 1>, true});
    // the 16x16x64 form at the same wave tile (scan_qs.h, M16): four private segments per workgroup and query
    vars.push_back({"qs16 RB2 SL6 NS3 noXPF NBUF8 PP1", 4, launch_qs<6, 2, 6, 3, false, 8, 0, 1, 0, 0, 1>, true});
    vars.push_back({"qs16 RB2 SL6 NS3 noXPF NBUF8", 4, launch_qs<6, 2, 6, 3, false, 8, 0, 0, 0, 0, 1>, true});
    vars.push_back({"qs2 4w x 64q RB2 NS3 NBUF8", 2, launch_qs2<6, 2, 3, 8, 0>, true});
    vars.push_back({"qs2 4w x 64q RB2 NS3 NBUF12", 2, launch_qs2<6, 2, 3, 12, 0>, true});
    vars.push_back({"qs2 4w x 64q RB1 NS6 NBUF8", 2, launch_qs2<6, 1, 6, 8, 0>, true});
#ifdef LYNSE_EXPERIMENTS
    vars.push_back({"qs RB1 SL6 NS6 XPF NBUF8 | no epilogue", 2, launch_qs<6, 1, 6, 6, true, 8, 16>, true});
    vars.push_back({"qs RB1 SL6 NS6 XPF NBUF8 | MFMA only", 2, launch_qs<6, 1, 6, 6, true, 8, 16 + 8 + 2>, true});
    vars.push_back({"qs RB1 SL6 NS6 XPF NBUF8 | MFMA + LDS reads", 2, launch_qs<6, 1, 6, 6, true, 8, 16 + 8>, true});
    vars.push_back({"qs RB1 SL6 NS6 XPF NBUF8 | DMA only", 2, launch_qs<6, 1, 6, 6, true, 8, 16 + 2 + 1>, true});
    vars.push_back({"qs RB1 SL6 NS6 XPF NBUF8 | DMA + LDS reads", 2, launch_qs<6, 1, 6, 6, true, 8, 16 + 1>, true});
    vars.push_back({"qs RB1 SL6 NS6 XPF NBUF8 | DMA + MFMA", 2, launch_qs<6, 1, 6, 6, true, 8, 16 + 2>, true});
    vars.push_back({"qs RB1 SL6 NS6 XPF NBUF8 | LDS reads only", 2, launch_qs<6, 1, 6, 6, true, 8, 16 + 8 + 1>, true});
    vars.push_back({"qs RB1 SL6 NS6 XPF NBUF8 | phase timing", 2, launch_qs<6, 1, 6, 6, true, 8, 32>, true});
    vars.push_back({"qs RB1 SL6 NS6 XPF NBUF8 PP1 | phase timing", 2, launch_qs<6, 1, 6, 6, true, 8, 32, 1>, true});
    vars.push_back({"qs RB1 SL6 NS6 XPF NBUF8 PP1 | no epilogue", 2, launch_qs<6, 1, 6, 6, true, 8, 16, 1>, true});
    vars.push_back({"qs RB2 SL6 NS3 noXPF NBUF8 STS | no emission", 2, launch_qs<6, 2, 6, 3, false, 8, 0, 0, 1>, true});
    vars.push_back({"qs RB2 SL6 NS3 noXPF NBUF8 STS | no emission noseedkernel", 2, launch_qs<6, 2, 6, 3, false, 8, 0, 0, 1>, true});
    vars.push_back({"qs RB2 SL6 NS3 noXPF NBUF8 PP1 STS | no emission noseedkernel", 2, launch_qs<6, 2, 6, 3, false, 8, 0, 1, 1>, true});
    vars.push_back({"qs RB2 SL6 NS3 noXPF NBUF8 PP1 | no emission", 2, launch_qs<6, 2, 6, 3, false, 8, 0, 1, 0>, true});
    vars.push_back({"qs RB2 SL6 NS3 noXPF NBUF8 | no emission", 2, launch_qs<6, 2, 6, 3, false, 8, 0, 0, 0>, true});
    vars.push_back({"qs RB1 SL6 NS6 | lone wave, MFMA only", 2, launch_qs<6, 1, 6, 6, true, 8, 64 + 16 + 8 + 2>, true});
    vars.push_back({"qs RB2 SL3 NS6 | lone wave, MFMA only", 2, launch_qs<6, 2, 3, 6, true, 8, 64 + 16 + 8 + 2>, true});
    vars.push_back({"qs RB1 SL6 NS6 | lone wave, MFMA + LDS reads", 2, launch_qs<6, 1, 6, 6, true, 8, 64 + 16 + 8>, true});
    vars.push_back({"qs RB2 SL3 NS6 | lone wave, MFMA + LDS reads", 2, launch_qs<6, 2, 3, 6, true, 8, 64 + 16 + 8>, true});
    vars.push_back({"qs RB1 SL6 NS6 | lone wave, MFMA + LDS + DMA", 2, launch_qs<6, 1, 6, 6, true, 8, 64 + 16>, true});
    vars.push_back({"qs RB2 SL3 NS6 | lone wave, MFMA + LDS + DMA", 2, launch_qs<6, 2, 3, 6, true, 8, 64 + 16>, true});
    vars.push_back({"old<2,4,4,2> | no epilogue", 4, launch_old<false, 16>, false});
    vars.push_back({"qs RB2 SL6 NS3 PP1 | no epilogue", 2, launch_qs<6, 2, 6, 3, false, 8, 16, 1>, true});
    vars.push_back({"qs RB2 SL6 NS3 PP1 | MFMA only 32x32x32", 2, launch_qs<6, 2, 6, 3, false, 8, 16 + 8 + 2, 1>, true});
    vars.push_back({"qs16 RB2 SL6 NS3 PP1 | no epilogue", 4, launch_qs<6, 2, 6, 3, false, 8, 16, 1, 0, 0, 1>, true});
    vars.push_back({"qs16 RB2 SL6 NS3 PP1 | MFMA only 16x16x64", 4, launch_qs<6, 2, 6, 3, false, 8, 16 + 8 + 2, 1, 0, 0, 1>, true});
    vars.push_back({"qs16 RB2 SL6 NS3 PP1 | MFMA + LDS reads", 4, launch_qs<6, 2, 6, 3, false, 8, 16 + 8, 1, 0, 0, 1>, true});
    vars.push_back({"qs16 RB2 SL6 NS3 PP1 | DMA + MFMA", 4, launch_qs<6, 2, 6, 3, false, 8, 16 + 2, 1, 0, 0, 1>, true});
    vars.push_back({"qs RB2 SL6 NS3 PP1 | MFMA + LDS reads", 2, launch_qs<6, 2, 6, 3, false, 8, 16 + 8, 1>, true});
    vars.push_back({"qs RB2 SL6 NS3 PP1 | DMA + MFMA", 2, launch_qs<6, 2, 6, 3, false, 8, 16 + 2, 1>, true});
    vars.push_back({"qs RB2 SL6 NS3 PP1 | DMA only", 2, launch_qs<6, 2, 6, 3, false, 8, 16 + 2 + 1, 1>, true});
    vars.push_back({"qs2 4w x 64q RB2 NS3 NBUF8 | no epilogue", 2, launch_qs2<6, 2, 3, 8, 16>, true});
    vars.push_back({"qs2 4w x 64q RB2 NS3 NBUF8 | MFMA only", 2, launch_qs2<6, 2, 3, 8, 16 + 8 + 2>, true});
    vars.push_back({"qs2 4w x 64q RB2 NS3 NBUF8 | MFMA + LDS reads", 2, launch_qs2<6, 2, 3, 8, 16 + 8>, true});
    vars.push_back({"qs2 4w x 64q RB2 NS3 NBUF8 | DMA + MFMA", 2, launch_qs2<6, 2, 3, 8, 16 + 2>, true});
    vars.push_back({"qs2 4w x 64q RB2 NS3 NBUF8 | phase timing qs2", 2, launch_qs2<6, 2, 3, 8, 32>, true});
    vars.push_back({"qs2 4w x 64q RB2 NS3 NBUF8 | MFMA + LDS reads, phase timing qs2", 2, launch_qs2<6, 2, 3, 8, 32 + 16 + 8>, true});
    vars.push_back({"qs2 4w x 64q RB2 NS3 NBUF8 | LDS reads only", 2, launch_qs2<6, 2, 3, 8, 16 + 8 + 1>, true});
    vars.push_back({"qs RB2 SL6 NS3 PP1 | LDS reads only", 2, launch_qs<6, 2, 6, 3, false, 8, 16 + 8 + 1, 1>, true});
#endif

    auto clear = [&](uint32_t nseg) {
        CK(hipMemsetAsync(b.count, 0, NQ * 4, 0));
        CK(hipMemsetAsync(b.segcnt, 0, (size_t)NQ * 4096, 0));
        (void)nseg;
    };


    // ---- 0. operand-distribution axis (first argument "operand"): the library's default instantiation, everything / no emission, over
    // row bytes (a) uniform [-128,127] (b) uniform [0,127] (c) uniform [0,63] (d) constant, and query images in [0,127] / [-127,127].
    // Same protocol as section 2 (long_warm launches of the SAME cell, then long_reps timed, `rounds` rounds kept after one discarded);
    // thresholds per query at mean + sigma_tight sd of ITS dot products over the rows, so every cell emits the same sparse share.
    if (operand_axis) {
        struct Dist { const char* name; uint32_t and_mask, or_bits; double mean, var; };
        const Dist dists[4] = {{"(a) rows uniform [-128,127]", 0xffffffffu, 0u, -0.5, (65536.0 - 1.0) / 12.0},
                               {"(b) rows uniform [0,127]", 0x7f7f7f7fu, 0u, 63.5, (16384.0 - 1.0) / 12.0},
                               {"(c) rows uniform [0,63]", 0x3f3f3f3fu, 0u, 31.5, (4096.0 - 1.0) / 12.0},
                               {"(d) rows constant 0x55", 0u, 0x55555555u, 85.0, 0.0}};
        const char* qkinds[2] = {"queries [0,127]", "queries [-127,127]"};
        const Variant* two[2] = {nullptr, nullptr};
        for (const Variant& v : vars) {
            if (v.name == "qs RB2 SL6 NS3 noXPF NBUF8 PP1") two[0] = &v;
            if (v.name == "qs RB2 SL6 NS3 noXPF NBUF8 PP1 | no emission") two[1] = &v;
        }
        if (!two[0] || !two[1]) { fprintf(stderr, "the operand axis needs -DLYNSE_EXPERIMENTS (the no-emission row)\n"); return 2; }
        const uint32_t n = (uint32_t)n_big;
        auto fill = [&](const Dist& d, bool nonneg) {
            hipLaunchKernelGGL(k_fill_rows, dim3(ncu * 8), dim3(256), 0, 0, b.V, n_big * D, 7ull, d.and_mask, d.or_bits);
            hipLaunchKernelGGL(k_fill_queries, dim3(QPAD), dim3(256), 0, 0, b.Qp, b.img, NQ, QPAD, D, NSLABS, nonneg);
            CK(hipDeviceSynchronize());
        };
        auto set_thr_cell = [&](const Dist& d, bool nonneg, double sig) {   // T_q = mean_c sum(u) + sig sd_c |u| (+1: a constant shard emits nothing)
            std::vector<float> one(NQ, 1.0f), zero(NQ, 0.0f), th(NQ);
            std::vector<int> ti(NQ);
            for (uint32_t q = 0; q < NQ; ++q) {
                double su = 0.0, su2 = 0.0;
                for (uint32_t i = 0; i < D; ++i) { const double u = query_elem(q, i, nonneg); su += u; su2 += u * u; }
                th[q] = (float)(std::floor(d.mean * su + sig * std::sqrt(d.var * su2)) + 1.0);
                ti[q] = (int)th[q];
            }
            CK(hipMemcpy(b.qinv, one.data(), NQ * 4, hipMemcpyHostToDevice));
            CK(hipMemcpy(b.qn2, zero.data(), NQ * 4, hipMemcpyHostToDevice));
            CK(hipMemcpy(b.thr, th.data(), NQ * 4, hipMemcpyHostToDevice));
            CK(hipMemcpy(b.Ti, ti.data(), NQ * 4, hipMemcpyHostToDevice));
        };
        int bad0 = 0;
        // key sets against the brute-force kernel on a small ragged shard, every cell (the default instantiation)
        for (int di = 0; di < 4; ++di)
            for (int qk = 0; qk < 2; ++qk) {
                const uint32_t ns = 65536u + 37u;
                fill(dists[di], qk == 0);
                set_thr_cell(dists[di], qk == 0, 3.0);
                uint64_t* ref_d; uint32_t* ref_n;
                const uint32_t ref_cap = 4u << 20;
                CK(hipMalloc(&ref_d, (size_t)ref_cap * 8)); CK(hipMalloc(&ref_n, 4)); CK(hipMemset(ref_n, 0, 4));
                hipLaunchKernelGGL(k_ref, dim3((ns + 63) / 64), dim3(256), 0, 0, b.V, D, D, ns, b.Qp, NQ, b.Ti, ref_d, ref_n, ref_cap);
                CK(hipDeviceSynchronize());
                uint32_t rn; CK(hipMemcpy(&rn, ref_n, 4, hipMemcpyDeviceToHost));
                std::vector<uint64_t> ref(std::min(rn, ref_cap));
                CK(hipMemcpy(ref.data(), ref_d, ref.size() * 8, hipMemcpyDeviceToHost));
                std::sort(ref.begin(), ref.end());
                CK(hipFree(ref_d)); CK(hipFree(ref_n));
                ScanArgs a = base_args(b, 0, ns, NQ);
                a.nseg = ncu * two[0]->segs_per_wg;
                a.seg = std::min<uint32_t>(255u, SEG_KEYS / a.nseg);
                clear(a.nseg);
                two[0]->launch(a, ncu, 0);
                CK(hipDeviceSynchronize());
                const std::vector<uint64_t> got = collect(b, NQ, a.nseg, a.seg);
                const bool ok = got == ref;
                bad0 += !ok;
                printf("check %-28s %-20s n %u sigma 3.0: %zu reference keys, %zu scanned%s\n", dists[di].name, qkinds[qk], ns, ref.size(), got.size(), ok ? "" : "   <-- MISMATCH");
            }
        struct Cell { std::vector<float> ms; double clk = 0, watts = 0, smhz = 0, keys = -1; };
        Cell cells[4][2][2];
        hipEvent_t e0, e1;
        CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
        for (int r = 0; r < rounds + 1; ++r)
            for (int di = 0; di < 4; ++di)
                for (int qk = 0; qk < 2; ++qk) {
                    fill(dists[di], qk == 0);
                    set_thr_cell(dists[di], qk == 0, sigma_tight);
                    for (int vi = 0; vi < 2; ++vi) {
                        const Variant& v = *two[vi];
                        Cell& c = cells[di][qk][vi];
                        ScanArgs a = base_args(b, 0, n, NQ);
                        a.nseg = ncu * v.segs_per_wg;
                        a.seg = std::min<uint32_t>(255u, SEG_KEYS / a.nseg);
                        a.debug_flags = 64 | (vi == 1 ? 2 : 0); a.dbg = b.dbg;
                        for (int w = 0; w < long_warm; ++w) { if (w < 2) clear(a.nseg); v.launch(a, ncu, 0); }
                        clear(a.nseg);
                        CK(hipDeviceSynchronize());
                        sampler.begin();
                        CK(hipEventRecord(e0, 0));
                        for (int i = 0; i < long_reps; ++i) v.launch(a, ncu, 0);
                        CK(hipEventRecord(e1, 0));
                        CK(hipEventSynchronize(e1));
                        { double pw, mz; sampler.end(&pw, &mz); if (r == rounds) { c.watts = pw; c.smhz = mz; } }
                        float t; CK(hipEventElapsedTime(&t, e0, e1));
                        if (r > 0) c.ms.push_back(t / long_reps);
                        unsigned long long tk[2];
                        CK(hipMemcpy(tk, b.dbg, 16, hipMemcpyDeviceToHost));
                        c.clk = (double)(tk[1] - tk[0]) / (t / long_reps * 1e3);
                        if (r == rounds && vi == 0) {   // keys one launch emits per query
                            clear(a.nseg); v.launch(a, ncu, 0);
                            CK(hipDeviceSynchronize());
                            const auto per = collect_q(b, NQ, a.nseg, a.seg);
                            size_t tot = 0;
                            for (auto& pq : per) tot += pq.size();
                            c.keys = (double)tot / NQ;
                        }
                    }
                }
        printf("---- operand axis: %u rows x %u B, %u queries, thresholds at %.1f sd; us per launch: median / min / spread (max - min) of %d rounds of %d launches behind %d warm-up launches\n",
               n, D, NQ, sigma_tight, rounds, long_reps, long_warm);
        double med_of[4][2][2], spread_of[4][2][2];
        for (int vi = 0; vi < 2; ++vi) {
            printf("-- %s\n", vi == 0 ? "everything" : "no emission");
            for (int di = 0; di < 4; ++di)
                for (int qk = 0; qk < 2; ++qk) {
                    Cell& c = cells[di][qk][vi];
                    std::sort(c.ms.begin(), c.ms.end());
                    const double med = c.ms[c.ms.size() / 2] * 1e3, mn = c.ms.front() * 1e3, sp = (c.ms.back() - c.ms.front()) * 1e3;
                    med_of[di][qk][vi] = med; spread_of[di][qk][vi] = sp;
                    printf("%-28s %-20s %8.1f %8.1f %7.1f   %5.2f TB/s   %6.0f MHz   hwmon %6.0f W %6.0f MHz", dists[di].name, qkinds[qk], med, mn, sp, (double)n * D / med / 1e6, c.clk, c.watts, c.smhz);
                    if (c.keys >= 0) printf("   %.0f keys per query", c.keys);
                    printf("\n");
                }
        }
        for (int vi = 0; vi < 2; ++vi) {
            const double gain = med_of[0][0][vi] - med_of[1][0][vi], need = 3.0 * spread_of[0][0][vi];
            printf("DECISION (%s, queries [0,127]): (a) %.1f us - (b) %.1f us = %.1f us; three times the spread of (a)'s rounds = %.1f us -> %s\n", vi == 0 ? "everything" : "no emission",
                   med_of[0][0][vi], med_of[1][0][vi], gain, need, gain > need ? "CONTINUE" : "STOP");
        }
        sampler.finish();
        printf("mismatches: %d\n", bad0);
        return bad0 ? 1 : 0;
    }

    // ---- 1. correctness on a small shard with a ragged end, two query counts, two thresholds, full and starved segments
    int bad = 0;
    for (int pass = 0; pass < 4 && only < 0; ++pass) {
        const uint32_t n = pass == 1 ? 8191u + 13u : 65536u + 37u, nq = pass == 2 ? 200u : 256u;
        const double sig = pass == 3 ? 1.6 : 3.0;
        set_thr(sig, nq);
        uint64_t* ref_d; uint32_t* ref_n;
        const uint32_t ref_cap = 4u << 20;
        CK(hipMalloc(&ref_d, (size_t)ref_cap * 8)); CK(hipMalloc(&ref_n, 4)); CK(hipMemset(ref_n, 0, 4));
        hipLaunchKernelGGL(k_ref, dim3((n + 63) / 64), dim3(256), 0, 0, b.V, D, D, n, b.Qp, nq, b.Ti, ref_d, ref_n, ref_cap);
        CK(hipDeviceSynchronize());
        uint32_t rn; CK(hipMemcpy(&rn, ref_n, 4, hipMemcpyDeviceToHost));
        std::vector<uint64_t> ref(std::min(rn, ref_cap));
        CK(hipMemcpy(ref.data(), ref_d, ref.size() * 8, hipMemcpyDeviceToHost));
        std::sort(ref.begin(), ref.end());
        CK(hipFree(ref_d)); CK(hipFree(ref_n));
        std::vector<uint64_t> ref_l2;
        {
            set_thr_l2(sig, nq);
            uint64_t* rd; uint32_t* rn2;
            const uint32_t rc = 4u << 20;
            CK(hipMalloc(&rd, (size_t)rc * 8)); CK(hipMalloc(&rn2, 4)); CK(hipMemset(rn2, 0, 4));
            hipLaunchKernelGGL(k_ref, dim3((n + 63) / 64), dim3(256), 0, 0, b.V, D, D, n, b.Qp, nq, b.Ti, rd, rn2, rc, b.vn2, b.qinv, b.qn2, b.thr);
            CK(hipDeviceSynchronize());
            uint32_t rnn; CK(hipMemcpy(&rnn, rn2, 4, hipMemcpyDeviceToHost));
            ref_l2.resize(std::min(rnn, rc));
            CK(hipMemcpy(ref_l2.data(), rd, ref_l2.size() * 8, hipMemcpyDeviceToHost));
            std::sort(ref_l2.begin(), ref_l2.end());
            CK(hipFree(rd)); CK(hipFree(rn2));
            set_thr(sig, nq);
        }
        for (size_t vi = 0; vi < vars.size(); ++vi) {
            const Variant& v = vars[vi];
            if (v.name.find('|') != std::string::npos) continue;
            if (qs16_axis && v.name.rfind("qs16", 0) != 0 && v.name != "qs RB2 SL6 NS3 noXPF NBUF8 PP1") continue;
            const bool l2v = v.name.rfind("L2", 0) == 0;
            if (l2v) set_thr_l2(sig, nq);
            struct Restore { std::function<void()> f; ~Restore() { f(); } } restore{[&]() { if (l2v) set_thr(sig, nq); }};
            const std::vector<uint64_t>& ref_use = l2v ? ref_l2 : ref;
            if (v.name.find("STS") != std::string::npos) {
                // self-tightening thresholds: the emitted set depends on timing; it must hold every (query, row) with
                // dot >= final tau - margin, only true scores, no duplicates, and tau must be reached by >= ks rows
                if (pass != 0 && pass != 2) continue;
                const int marg = (int)(0.5 * sd);
                int* dots; CK(hipMalloc(&dots, (size_t)nq * n * 4));
                hipLaunchKernelGGL(k_all_dots, dim3((n + 63) / 64), dim3(256), 0, 0, b.V, D, D, n, b.Qp, nq, dots);
                std::vector<int> hd((size_t)nq * n);
                CK(hipMemcpy(hd.data(), dots, hd.size() * 4, hipMemcpyDeviceToHost));
                CK(hipFree(dots));
                for (int starve = 0; starve < 2; ++starve) {
                    ScanArgs a = base_args(b, 0, n, nq);
                    const uint32_t grid = std::min((n + 31) / 32, ncu);
                    a.nseg = grid * v.segs_per_wg;
                    a.seg = starve ? 4u : std::min<uint32_t>(255u, SEG_KEYS / a.nseg);
                    clear(a.nseg);
                    hipLaunchKernelGGL(k_seed, dim3(nq), dim3(256), 0, 0, b.V, D, D, n, b.Qp, 64u, a.dyn_ks, 320u, b.dyn_thr, b.dyn_slot, b.dyn_marg, marg);
                    v.launch(a, ncu, 0);
                    CK(hipDeviceSynchronize());
                    const auto per = collect_q(b, nq, a.nseg, a.seg);
                    std::vector<int> tau(nq);
                    CK(hipMemcpy(tau.data(), b.dyn_thr, nq * 4, hipMemcpyDeviceToHost));
                    size_t wrong = 0, dup = 0, missing = 0, weak = 0, expect = 0, got_n = 0;
                    std::vector<std::vector<uint32_t>> rows_of(nq);
                    for (uint32_t q = 0; q < nq; ++q)
                        for (uint64_t key : per[q]) {
                            ++got_n;
                            const uint32_t row = (uint32_t)(key & 0xffffffffu);
                            if (row < n && make_key((float)hd[(size_t)q * n + row], row, false) == key) rows_of[q].push_back(row);
                            else ++wrong;
                        }
                    std::vector<uint32_t> cnts(nq);
                    CK(hipMemcpy(cnts.data(), b.count, nq * 4, hipMemcpyDeviceToHost));
                    size_t overflowed = 0;
                    for (uint32_t q = 0; q < nq; ++q) {
                        if (cnts[q] > b.cap) { ++overflowed; continue; }   // (the library reruns such a query on the next plan)
                        std::sort(rows_of[q].begin(), rows_of[q].end());
                        for (size_t i = 1; i < rows_of[q].size(); ++i) dup += rows_of[q][i] == rows_of[q][i - 1];
                        size_t reach = 0;
                        for (uint32_t r = 0; r < n; ++r) {
                            const int d = hd[(size_t)q * n + r];
                            reach += d >= tau[q];
                            if (d >= tau[q] - marg) { ++expect; if (!std::binary_search(rows_of[q].begin(), rows_of[q].end(), r)) ++missing; }
                        }
                        weak += reach < a.dyn_ks;
                    }
                    const bool ok = !wrong && !dup && !missing && !weak;
                    if (!ok) ++bad;
                    printf("STS pass %d %-36s starve %d: %zu keys emitted, %zu required; wrong %zu dup %zu missing %zu taus-not-reached %zu overflowed-queries %zu%s\n", pass, v.name.c_str(), starve,
                           got_n, expect, wrong, dup, missing, weak, overflowed, ok ? "" : "   <-- MISMATCH");
                }
                continue;
            }
            for (int starve = 0; starve < 2; ++starve) {
                ScanArgs a = base_args(b, 0, n, nq);
                const uint32_t tiles = v.qs ? (n + 31) / 32 : (n + 255) / 256;   // (an upper bound of the grid is enough for nseg)
                const uint32_t grid = std::min(tiles, ncu);
                a.nseg = grid * v.segs_per_wg;
                a.seg = starve ? 2u : std::min<uint32_t>(255u, SEG_KEYS / a.nseg);
                clear(a.nseg);
                v.launch(a, ncu, 0);
                CK(hipDeviceSynchronize());
                std::vector<uint64_t> got = collect(b, nq, a.nseg, a.seg);
                const std::vector<uint64_t>& ref = ref_use;
                const bool ok = got == ref;
                if (ok && qs16_axis) printf("ok       pass %d %-34s starve %d: %zu keys, identical to the brute-force set\n", pass, v.name.c_str(), starve, got.size());
                if (!ok) {
                    ++bad;
                    printf("MISMATCH pass %d %-34s starve %d: ref %zu keys, got %zu\n", pass, v.name.c_str(), starve, ref.size(), got.size());
                    size_t i = 0;
                    while (i < ref.size() && i < got.size() && ref[i] == got[i]) ++i;
                    if (i < ref.size()) printf("   first difference at %zu: ref q %u row %u", i, (unsigned)(ref[i] >> 48) , (unsigned)(ref[i] & 0xffffffffu));
                    if (i < got.size()) printf("  got q %u row %u", (unsigned)(got[i] >> 48), (unsigned)(got[i] & 0xffffffffu));
                    printf("\n");
                }
            }
        }
        printf("check pass %d: n %u nq %u sigma %.1f -> %zu reference keys (L2: %zu); mismatching variants so far %d\n", pass, n, nq, sig, ref.size(), ref_l2.size(), bad);
    }

    // ---- 1b. MFMA shape (first argument "qs16"): v_mfma_i32_32x32x32_i8 against v_mfma_i32_16x16x64_i8 at the same wave tile, everything and
    // the decompositions, on (b) SQ7-like operands (rows and query image in [0,127]) and (a) centred ones.  Protocol of section 0.
    if (qs16_axis) {
#ifndef LYNSE_EXPERIMENTS
        fprintf(stderr, "the qs16 axis needs -DLYNSE_EXPERIMENTS (the decomposition rows)\n");
        return 2;
#else
        struct Op { const char* name; uint32_t and_mask; bool nonneg; double mean, var; };
        const Op ops[2] = {{"(b) rows [0,127], queries [0,127]", 0x7f7f7f7fu, true, 63.5, (16384.0 - 1.0) / 12.0},
                           {"(a) rows [-128,127], queries [-127,127]", 0xffffffffu, false, -0.5, (65536.0 - 1.0) / 12.0}};
        const char* names[8] = {"qs RB2 SL6 NS3 noXPF NBUF8 PP1", "qs16 RB2 SL6 NS3 noXPF NBUF8 PP1",
                                "qs RB2 SL6 NS3 PP1 | MFMA only 32x32x32", "qs16 RB2 SL6 NS3 PP1 | MFMA only 16x16x64",
                                "qs RB2 SL6 NS3 PP1 | MFMA + LDS reads", "qs16 RB2 SL6 NS3 PP1 | MFMA + LDS reads",
                                "qs RB2 SL6 NS3 PP1 | DMA + MFMA", "qs16 RB2 SL6 NS3 PP1 | DMA + MFMA"};
        const Variant* vs[8] = {};
        for (int i = 0; i < 8; ++i) {
            for (const Variant& v : vars) if (v.name == names[i]) vs[i] = &v;
            if (!vs[i]) { fprintf(stderr, "variant %s is not built\n", names[i]); return 2; }
        }
        const uint32_t n = (uint32_t)n_big;
        auto fill = [&](const Op& o) {
            hipLaunchKernelGGL(k_fill_rows, dim3(ncu * 8), dim3(256), 0, 0, b.V, n_big * D, 7ull, o.and_mask, 0u);
            hipLaunchKernelGGL(k_fill_queries, dim3(QPAD), dim3(256), 0, 0, b.Qp, b.img, NQ, QPAD, D, NSLABS, o.nonneg);
            CK(hipDeviceSynchronize());
        };
        auto set_thr_op = [&](const Op& o, double sig) {   // T_q = mean_c sum(u) + sig sd_c |u|
            std::vector<float> one(NQ, 1.0f), zero(NQ, 0.0f), th(NQ);
            std::vector<int> ti(NQ);
            for (uint32_t q = 0; q < NQ; ++q) {
                double su = 0.0, su2 = 0.0;
                for (uint32_t i = 0; i < D; ++i) { const double u = query_elem(q, i, o.nonneg); su += u; su2 += u * u; }
                th[q] = (float)(std::floor(o.mean * su + sig * std::sqrt(o.var * su2)) + 1.0);
                ti[q] = (int)th[q];
            }
            CK(hipMemcpy(b.qinv, one.data(), NQ * 4, hipMemcpyHostToDevice));
            CK(hipMemcpy(b.qn2, zero.data(), NQ * 4, hipMemcpyHostToDevice));
            CK(hipMemcpy(b.thr, th.data(), NQ * 4, hipMemcpyHostToDevice));
            CK(hipMemcpy(b.Ti, ti.data(), NQ * 4, hipMemcpyHostToDevice));
        };
        // key sets of both forms against the brute-force kernel on the SQ7-like operands too (the four passes above ran on the centred ones)
        {
            const uint32_t ns = 65536u + 37u;
            fill(ops[0]);
            set_thr_op(ops[0], 3.0);
            uint64_t* ref_d; uint32_t* ref_n;
            const uint32_t ref_cap = 4u << 20;
            CK(hipMalloc(&ref_d, (size_t)ref_cap * 8)); CK(hipMalloc(&ref_n, 4)); CK(hipMemset(ref_n, 0, 4));
            hipLaunchKernelGGL(k_ref, dim3((ns + 63) / 64), dim3(256), 0, 0, b.V, D, D, ns, b.Qp, NQ, b.Ti, ref_d, ref_n, ref_cap);
            CK(hipDeviceSynchronize());
            uint32_t rn; CK(hipMemcpy(&rn, ref_n, 4, hipMemcpyDeviceToHost));
            std::vector<uint64_t> ref(std::min(rn, ref_cap));
            CK(hipMemcpy(ref.data(), ref_d, ref.size() * 8, hipMemcpyDeviceToHost));
            std::sort(ref.begin(), ref.end());
            CK(hipFree(ref_d)); CK(hipFree(ref_n));
            for (int i = 0; i < 2; ++i) {
                ScanArgs a = base_args(b, 0, ns, NQ);
                a.nseg = ncu * vs[i]->segs_per_wg;
                a.seg = std::min<uint32_t>(255u, SEG_KEYS / a.nseg);
                clear(a.nseg);
                vs[i]->launch(a, ncu, 0);
                CK(hipDeviceSynchronize());
                const bool ok = collect(b, NQ, a.nseg, a.seg) == ref;
                bad += !ok;
                printf("check %-36s %-34s n %u sigma 3.0: %zu reference keys%s\n", ops[0].name, names[i], ns, ref.size(), ok ? ", identical" : "   <-- MISMATCH");
            }
        }
        struct Cell { std::vector<float> ms; double clk = 0, watts = 0, smhz = 0, ticks = 0; };
        Cell cells[2][8];
        hipEvent_t e0, e1;
        CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
        for (int r = 0; r < rounds + 1; ++r)
            for (int oi = 0; oi < 2; ++oi) {
                fill(ops[oi]);
                set_thr_op(ops[oi], sigma_tight);
                for (int vi = 0; vi < 8; ++vi) {
                    const Variant& v = *vs[vi];
                    Cell& c = cells[oi][vi];
                    ScanArgs a = base_args(b, 0, n, NQ);
                    a.nseg = ncu * v.segs_per_wg;
                    a.seg = std::min<uint32_t>(255u, SEG_KEYS / a.nseg);
                    a.debug_flags = 64; a.dbg = b.dbg;
                    for (int w = 0; w < long_warm; ++w) { if (w < 2) clear(a.nseg); v.launch(a, ncu, 0); }
                    clear(a.nseg);
                    CK(hipDeviceSynchronize());
                    sampler.begin();
                    CK(hipEventRecord(e0, 0));
                    for (int i = 0; i < long_reps; ++i) v.launch(a, ncu, 0);
                    CK(hipEventRecord(e1, 0));
                    CK(hipEventSynchronize(e1));
                    { double pw, mz; sampler.end(&pw, &mz); if (r == rounds) { c.watts = pw; c.smhz = mz; } }
                    float t; CK(hipEventElapsedTime(&t, e0, e1));
                    if (r > 0) c.ms.push_back(t / long_reps);
                    unsigned long long tk[2];
                    CK(hipMemcpy(tk, b.dbg, 16, hipMemcpyDeviceToHost));
                    c.ticks = (double)(tk[1] - tk[0]);
                    c.clk = c.ticks / (t / long_reps * 1e3);
                }
            }
        // MFMAs one SIMD issues in a launch of workgroup 0: its tiles x 48 (32x32x32) or 96 (16x16x64) per wave, two waves per SIMD
        const double tiles0 = std::ceil((double)((n + 63) / 64) / ncu);
        printf("---- MFMA shape: %u rows x %u B, %u queries, thresholds at %.1f sd; us per launch: median / min / spread of %d rounds of %d launches behind %d warm-up launches;\n"
               "     s_memtime MHz = shader cycles of workgroup 0 / launch time; cyc/MFMA = those cycles / (MFMAs its SIMD issued: %.0f tiles x 48 or 96 x 2 waves)\n",
               n, D, NQ, sigma_tight, rounds, long_reps, long_warm, tiles0);
        for (int oi = 0; oi < 2; ++oi) {
            printf("-- %s\n", ops[oi].name);
            double med_of[8], sp_of[8];
            for (int vi = 0; vi < 8; ++vi) {
                Cell& c = cells[oi][vi];
                std::sort(c.ms.begin(), c.ms.end());
                const double med = c.ms[c.ms.size() / 2] * 1e3, mn = c.ms.front() * 1e3, sp = (c.ms.back() - c.ms.front()) * 1e3;
                med_of[vi] = med; sp_of[vi] = sp;
                printf("%-46s %8.1f %8.1f %7.1f   %6.0f MHz   hwmon %6.0f W %6.0f MHz   %6.1f cyc/MFMA\n", names[vi], med, mn, sp, c.clk, c.watts, c.smhz,
                       c.ticks / (tiles0 * ((vi & 1) ? 96.0 : 48.0) * 2.0));
            }
            const double gain = med_of[0] - med_of[1], need = 3.0 * std::max(sp_of[0], sp_of[1]);
            printf("GATE %s: 32x32x32 %.1f us - 16x16x64 %.1f us = %.1f us; three times the larger spread = %.1f us -> %s\n", ops[oi].name, med_of[0], med_of[1], gain, need,
                   gain > need ? "16x16x64 WINS" : "no gain");
        }
        sampler.finish();
        printf("mismatches: %d\n", bad);
        return bad ? 1 : 0;
#endif
    }

    // ---- 2. timing
    for (double sig : {sigma_tight, sigma_loose}) {
        set_thr(sig, NQ);
        const uint32_t n = (uint32_t)n_big;
        bool prev_l2 = false;
        std::vector<std::vector<float>> ms(vars.size());
        std::vector<double> clk(vars.size(), 0.0), watts(vars.size(), 0.0), smhz(vars.size(), 0.0);
        hipEvent_t e0, e1;
        CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
        for (int r = 0; r < rounds + 1; ++r) {
            for (size_t vi = 0; vi < vars.size(); ++vi) {
                if (only >= 0 && (int)vi != only) continue;
                const Variant& v = vars[vi];
                ScanArgs a = base_args(b, 0, n, NQ);
                a.nseg = ncu * v.segs_per_wg;
                a.seg = std::min<uint32_t>(255u, SEG_KEYS / a.nseg);
                a.debug_flags = 64; a.dbg = b.dbg;
                if (v.name.find("no emission") != std::string::npos) a.debug_flags |= 2;
                if (v.name.find("nowarm") != std::string::npos) a.dyn_warm = 0;
                if (v.name.find("norefresh") != std::string::npos) a.debug_flags |= 256;
                const int reps = long_reps;
                const bool l2v = v.name.rfind("L2", 0) == 0;
                if (l2v) set_thr_l2(sig, NQ); else if (prev_l2) set_thr(sig, NQ);
                prev_l2 = l2v;
                const bool sts = v.name.find("STS") != std::string::npos;
                const bool noseed = v.name.find("noseedkernel") != std::string::npos;
                // (the stand-in seed kernel of this tool costs ~80 us; the library seeds inside k_i8c_prep_queries.  Timed STS runs restore the
                // seeded state with three small copies instead)
                const bool fastseed = sts && !noseed;
                static int *seed_thr = nullptr, *seed_slot = nullptr;
                if (fastseed) {
                    if (!seed_thr) { CK(hipMalloc(&seed_thr, NQ * 4)); CK(hipMalloc(&seed_slot, NQ * 32 * 4)); }
                    hipLaunchKernelGGL(k_seed, dim3(NQ), dim3(256), 0, 0, b.V, D, D, n, b.Qp, 64u, a.dyn_ks, 320u, b.dyn_thr, b.dyn_slot, b.dyn_marg, (int)(sts_marg_sd * sd));
                    CK(hipMemcpyAsync(seed_thr, b.dyn_thr, NQ * 4, hipMemcpyDeviceToDevice, 0));
                    CK(hipMemcpyAsync(seed_slot, b.dyn_slot, NQ * 32 * 4, hipMemcpyDeviceToDevice, 0));
                }
                auto reseed = [&]() {
                    if (!fastseed) return;
                    CK(hipMemcpyAsync(b.dyn_thr, seed_thr, NQ * 4, hipMemcpyDeviceToDevice, 0));
                    CK(hipMemcpyAsync(b.dyn_slot, seed_slot, NQ * 32 * 4, hipMemcpyDeviceToDevice, 0));
                };
                auto seed = [&]() { if (sts && !noseed && !fastseed) hipLaunchKernelGGL(k_seed, dim3(NQ), dim3(256), 0, 0, b.V, D, D, n, b.Qp, 64u, a.dyn_ks, 320u, b.dyn_thr, b.dyn_slot, b.dyn_marg, (int)(sts_marg_sd * sd)); };
                for (int w = 0; w < long_warm; ++w) { if (w < 2) clear(a.nseg); seed(); reseed(); v.launch(a, ncu, 0); }   // warm: clocks / power settle under THIS variant
                clear(a.nseg);
                CK(hipDeviceSynchronize());
                const auto w0 = std::chrono::system_clock::now();
                sampler.begin();
                CK(hipEventRecord(e0, 0));
                for (int i = 0; i < reps; ++i) { seed(); reseed(); v.launch(a, ncu, 0); }
                CK(hipEventRecord(e1, 0));
                CK(hipEventSynchronize(e1));
                const auto w1 = std::chrono::system_clock::now();
                { double pw, mz; sampler.end(&pw, &mz); if (r == rounds) { watts[vi] = pw; smhz[vi] = mz; } }
                float t; CK(hipEventElapsedTime(&t, e0, e1));
                if (r > 0) ms[vi].push_back(t / reps);
                if (v.qs) {
                    unsigned long long tk[2];
                    CK(hipMemcpy(tk, b.dbg, 16, hipMemcpyDeviceToHost));
                    clk[vi] = (double)(tk[1] - tk[0]) / (t / reps * 1e3);   // ticks per microsecond = MHz (kernel span of workgroup 0 ~ launch)
                }
                if (r == rounds && sts && v.name.find("no emission") == std::string::npos) {   // how many keys the launch emitted per query
                    clear(a.nseg); reseed(); seed(); v.launch(a, ncu, 0);
                    CK(hipDeviceSynchronize());
                    const auto per = collect_q(b, NQ, a.nseg, a.seg);
                    size_t mx = 0, tot = 0;
                    for (auto& pq : per) { mx = std::max(mx, pq.size()); tot += pq.size(); }
                    std::vector<uint32_t> cnts(NQ);
                    CK(hipMemcpy(cnts.data(), b.count, NQ * 4, hipMemcpyDeviceToHost));
                    uint32_t cmax = 0; for (uint32_t c : cnts) cmax = std::max(cmax, c);
                    printf("KEYS %s: %.0f per query on average, %zu at most; shared-region count at most %u (cap %u), segment slots %u\n", v.name.c_str(), (double)tot / NQ, mx, cmax, b.cap, a.seg);
                }
                if (r == rounds && v.name.find("phase timing qs2") != std::string::npos) {
                    std::vector<unsigned long long> ph(64 * 4 * 4);
                    CK(hipMemcpy(ph.data(), b.dbg + 4096, ph.size() * 8, hipMemcpyDeviceToHost));
                    printf("PHASE %s\n", v.name.c_str());
                    for (int blk : {0, 17}) {
                        for (int w = 0; w < 4; ++w) {
                            const unsigned long long* o = ph.data() + ((size_t)blk * 4 + w) * 4;
                            const double tot = (double)(o[0] + o[1] + o[2] + o[3]);
                            const double steps = (double)((n + 63) / 64) / ncu;
                            printf("PHASE block %2d wave %d: per step  wait %6.0f  barrier %6.0f  loop %6.0f  epilogue+issue %6.0f  (sum %.0f ticks)\n", blk, w,
                                   o[0] / steps, o[1] / steps, o[2] / steps, o[3] / steps, tot / steps);
                        }
                    }
                } else
                if (r == rounds && v.name.find("phase timing") != std::string::npos) {
                    std::vector<unsigned long long> ph(64 * 8 * 4);
                    CK(hipMemcpy(ph.data(), b.dbg + 512, ph.size() * 8, hipMemcpyDeviceToHost));
                    printf("PHASE %s\n", v.name.c_str());
                    for (int blk : {0, 17}) {
                        for (int w = 0; w < 8; ++w) {
                            const unsigned long long* o = ph.data() + ((size_t)blk * 8 + w) * 4;
                            const double tot = (double)(o[0] + o[1] + o[2] + o[3]);
                            printf("PHASE block %2d wave %d: wait %5.1f%% barrier %5.1f%% loop %5.1f%% epilogue %5.1f%%  (%.0f cycles, %.0f per step)\n", blk, w,
                                   100.0 * o[0] / tot, 100.0 * o[1] / tot, 100.0 * o[2] / tot, 100.0 * o[3] / tot, tot, tot / ((double)((n + 31) / 32) / ncu));
                        }
                    }
                }
                if (r == rounds)
                    printf("STAMP %-44s %.6f %.6f\n", v.name.c_str(), std::chrono::duration<double>(w0.time_since_epoch()).count(),
                           std::chrono::duration<double>(w1.time_since_epoch()).count());
            }
        }
        printf("---- %u rows x %u B, %u queries, thresholds at %.1f sd: us per launch (median / min of %d rounds), TB/s of codes, s_memtime MHz\n",
               n, D, NQ, sig, rounds);
        for (size_t vi = 0; vi < vars.size(); ++vi) {
            if (ms[vi].empty()) continue;
            std::sort(ms[vi].begin(), ms[vi].end());
            const double med = ms[vi][ms[vi].size() / 2] * 1e3, mn = ms[vi][0] * 1e3;
            printf("%-46s %8.1f %8.1f   %5.2f TB/s   %6.0f MHz   hwmon %6.0f W %6.0f MHz\n", vars[vi].name.c_str(), med, mn, (double)n * D / med / 1e6, clk[vi], watts[vi], smhz[vi]);
        }
    }
    sampler.finish();
    printf("mismatches: %d\n", bad);
    return bad ? 1 : 0;
}
