// llc_slice.hip -- can part of a streamed column live in the 256 MiB Infinity Cache from launch to launch?  (gate experiment)
//
// The equality scan at 1e9 x 9 bit reads 9 KiB and writes 1 KiB per wave tile with non-temporal LDS-DMA loads, at the rate a
// copy achieves from HBM.  This tool keeps the scan's shape (one LDS buffer per wave: wait, ds_read, issue the next tile's DMA,
// K = 4 tiles per store burst, one block per CU) and varies only the cache policy of the loads, per tile and by address:
//   a tile whose first byte lies in a RESIDENT 64 KiB granule is loaded with the default policy (aux 0), every other tile
//   non-temporal (aux 2).  Resident granules are either a contiguous head of the source ("head") or every D-th granule
//   ("spread", g mod D == 0; D odd, so every wave meets the same share in every round of a power-of-two grid).
// Launches run back to back on the same source, so whatever survives in the cache from one launch serves the next.
// Questions: do nt loads leave resident lines alone, how much may be resident next to the bitmap (sc1 or nt stores), does the
// spread form beat the head, and what does it cost when two sources alternate (each one's granules evict the other's).
// Build: hipcc --offload-arch=gfx950 -O3 -std=c++17 tools/llc_slice.hip -o tools/llc_slice
// Run:   tools/llc_slice [launches per burst=50]
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

#define GPTR(p) ((const __attribute__((address_space(1))) void *)(p))
#define LPTR(p) ((__attribute__((address_space(3))) void *)(p))

#define CK(x)                                                                                 \
    do {                                                                                      \
        hipError_t e_ = (x);                                                                  \
        if (e_ != hipSuccess) {                                                               \
            fprintf(stderr, "%s:%d %s: %s\n", __FILE__, __LINE__, #x, hipGetErrorString(e_)); \
            exit(1);                                                                          \
        }                                                                                     \
    } while (0)

constexpr int R = 9;              // KiB read per step
constexpr int kGranuleShift = 16; // 64 KiB

template <int NTS> __device__ __forceinline__ void store16(u32x4 *p, u32x4 v)
{
    if constexpr (NTS == 2)
        asm volatile("global_store_dwordx4 %0, %1, off sc1" ::"v"(p), "v"(v) : "memory");
    else
        __builtin_nontemporal_store(v, p);
}

template <int AUX> __device__ __forceinline__ void dma_step(const uint8_t *src, uint8_t *lds_wave, int lane)
{
#pragma unroll
    for (int j = 0; j < R; j++)
        __builtin_amdgcn_global_load_lds(GPTR(src + j * 1024 + lane * 16), LPTR(lds_wave + j * 1024), 16, 0, AUX);
}

struct Slice {
    uint64_t head_bytes; // [0, head_bytes) is resident
    uint32_t D;          // 0: no spread granules, 1: everything, else granule g is resident iff g mod D == 0
};

__device__ __forceinline__ void issue(const uint8_t *src, uint64_t step, Slice s, uint8_t *lds_wave, int lane)
{
    const uint64_t off = step * (uint64_t)(R * 1024);
    const uint32_t g = (uint32_t)(off >> kGranuleShift);
    const bool resident = off < s.head_bytes || s.D == 1 || (s.D > 1 && g % s.D == 0); // wave-uniform
    if (resident)
        dma_step<0>(src + off, lds_wave, lane);
    else
        dma_step<2>(src + off, lds_wave, lane);
}

template <int K, int NTS> __global__ __launch_bounds__(256) void slice_kernel(const uint8_t *src, u32x4 *dst, uint64_t nchunks, Slice s)
{
    __shared__ __attribute__((aligned(16))) uint8_t lds[4][R * 1024];
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    uint8_t *lds_wave = lds[wv];
    const uint64_t stride = (uint64_t)gridDim.x * 4;
    uint64_t ch = (uint64_t)blockIdx.x * 4 + wv;
    u32x4 held[K];
    uint64_t held_chunk = ~0ull;
    bool have_held = false;
    if (ch < nchunks) issue(src, ch * K, s, lds_wave, lane);
    while (ch < nchunks) {
        u32x4 acc[K];
#pragma unroll
        for (int k = 0; k < K; k++) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            u32x4 a = {0, 0, 0, 0};
#pragma unroll
            for (int r = 0; r < R; r++) a ^= *(const u32x4 *)(lds_wave + r * 1024 + lane * 16);
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            if (k == 0 && have_held) { // the previous chunk's burst, in front of the next DMA (the scan's deferral)
                u32x4 *q = dst + held_chunk * K * 64 + lane;
#pragma unroll
                for (int i = 0; i < K; i++) store16<NTS>(q + i * 64, held[i]);
            }
            const uint64_t next = k + 1 < K ? ch * K + k + 1 : (ch + stride) * K;
            if (k + 1 < K || ch + stride < nchunks) issue(src, next, s, lds_wave, lane);
            acc[k] = a;
        }
#pragma unroll
        for (int k = 0; k < K; k++) held[k] = acc[k];
        held_chunk = ch;
        have_held = true;
        ch += stride;
    }
    if (have_held) {
        u32x4 *q = dst + held_chunk * K * 64 + lane;
#pragma unroll
        for (int i = 0; i < K; i++) store16<NTS>(q + i * 64, held[i]);
    }
}

struct Variant {
    std::string name;
    uint64_t rows;
    Slice s;
    int nts;  // 2 sc1, 1 nt
    int alt;  // launch by launch: 0 one source; 1 two sources and two destinations in turn (ALT); 2 two sources, one destination (ALT1)
    std::vector<float> ms;
};

int main(int argc, char **argv)
{
    const int BURST = argc > 1 ? atoi(argv[1]) : 50;
    constexpr int K = 4;
    hipDeviceProp_t prop;
    CK(hipGetDeviceProperties(&prop, 0));
    const int cus = prop.multiProcessorCount;
    const uint64_t max_rows = 1000000000ull;
    auto steps_of = [](uint64_t rows) { return rows * R / 8 / (R * 1024) / 64 * 64; }; // whole chunks
    const uint64_t max_steps = steps_of(max_rows);
    uint8_t *src[2];
    u32x4 *dst[2];
    for (int i = 0; i < 2; i++) {
        CK(hipMalloc(&src[i], max_steps * R * 1024 + 4096));
        CK(hipMalloc(&dst[i], max_steps * 1024 + 4096));
        CK(hipMemset(src[i], 0x5a + i, max_steps * R * 1024));
        CK(hipMemset(dst[i], 0, max_steps * 1024));
    }
    printf("device %s, %d CUs; steps of %d KiB read + 1 KiB written, K = %d, one block per CU, LDS-DMA loads\n", prop.gcnArchName, cus, R, K);

    const double MiB = 1048576.0;
    std::vector<Variant> vs;
    auto add = [&](uint64_t rows, const char *place, uint64_t head_mib, uint32_t D, int nts, int alt) {
        const double srcb = steps_of(rows) * R * 1024.0;
        const double res = D == 1 ? srcb : (D > 1 ? srcb / D : (double)std::min<double>(head_mib * MiB, srcb));
        char nm[128];
        snprintf(nm, sizeof nm, "rows=%.3g %-6s res=%6.1fMiB D=%-2u %s%s", (double)rows, place, res / MiB, D, nts == 2 ? "sc1" : "nt ",
                 alt == 1 ? " ALT" : alt == 2 ? " ALT1" : "");
        vs.push_back({nm, rows, Slice{head_mib << 20, D}, nts, alt, {}});
    };
    const uint64_t heads[] = {32, 64, 96, 112, 128, 160, 192, 224};
    const uint32_t Ds[] = {33, 17, 11, 9, 7, 5, 3}; // spread shares of 1073 MiB: 32.5, 63, 97.5, 119, 153, 215, 358 MiB
    for (int nts : {2, 1}) {
        add(max_rows, "off", 0, 0, nts, 0);
        for (uint64_t h : heads) add(max_rows, "head", h, 0, nts, 0);
        for (uint32_t D : Ds) add(max_rows, "spread", 0, D, nts, 0);
    }
    add(max_rows, "all", 0, 1, 2, 0); // everything default policy (dma_aux = 0)
    for (int alt : {1, 2})
        for (uint32_t D : {0u, 65u, 33u, 21u, 17u, 11u, 9u, 5u}) add(max_rows, D ? "spread" : "off", 0, D, 2, alt);
    for (uint32_t D : {0u, 17u, 11u, 7u, 5u}) add(max_rows, D ? "spread" : "off", 0, D, 1, 1);
    for (uint64_t rows : {500000000ull, 250000000ull, 125000000ull}) {
        add(rows, "off", 0, 0, 2, 0);
        add(rows, "off", 0, 0, 1, 0);
        for (uint32_t D : {9u, 7u, 5u, 3u}) add(rows, "spread", 0, D, 2, 0);
        add(rows, "head", 128, 0, 2, 0);
        if (rows <= 250000000ull) {
            add(rows, "all", 0, 1, 2, 0);
            add(rows, "all", 0, 1, 1, 0);
            add(rows, "all", 0, 1, 2, 1);
            add(rows, "off", 0, 0, 2, 1);
        }
    }

    auto launch = [&](const Variant &v, int w) {
        const uint64_t nchunks = steps_of(v.rows) / K;
        const int which = v.alt ? (w & 1) : 0, whichd = v.alt == 1 ? (w & 1) : 0;
        if (v.nts == 2)
            hipLaunchKernelGGL((slice_kernel<K, 2>), dim3(cus), dim3(256), 0, 0, src[which], dst[whichd], nchunks, v.s);
        else
            hipLaunchKernelGGL((slice_kernel<K, 1>), dim3(cus), dim3(256), 0, 0, src[which], dst[whichd], nchunks, v.s);
    };
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0));
    CK(hipEventCreate(&e1));
    for (int round = 0; round < 5; round++)
        for (auto &v : vs) {
            for (int w = 0; w < 4; w++) launch(v, w);
            CK(hipDeviceSynchronize());
            CK(hipEventRecord(e0, 0));
            for (int w = 0; w < BURST; w++) launch(v, w);
            CK(hipEventRecord(e1, 0));
            CK(hipEventSynchronize(e1));
            CK(hipGetLastError());
            float ms;
            CK(hipEventElapsedTime(&ms, e0, e1));
            v.ms.push_back(ms / BURST);
        }
    printf("%-44s %9s %9s %9s %9s   rounds (ms per launch; %d launches back to back, 5 rounds, variants interleaved)\n", "variant", "median", "best",
           "worst", "read GB/s", BURST);
    for (auto &v : vs) {
        std::vector<float> t = v.ms;
        std::sort(t.begin(), t.end());
        printf("%-44s %9.4f %9.4f %9.4f %9.1f  ", v.name.c_str(), t[2], t[0], t[4], steps_of(v.rows) * R * 1024.0 / t[2] / 1e6);
        for (float x : v.ms) printf(" %.4f", x);
        printf("\n");
    }
    return 0;
}
