// microbench_smem.hip — dev tool: the round trip of a scalar load that hits the scalar data cache, one wave per SIMD,
// on gfx950: what k_optimize pays wherever it reloads a DevConst field and waits for it (profiles/README.md).
//   hipcc --offload-arch=gfx950 -O3 -o /tmp/mb_smem tools/microbench_smem.hip && /tmp/mb_smem
// The wave chases a pointer through a 256-byte block (32 qwords, each holding the address of another qword of the
// block, one cycle through all 32): s_load_dwordx2 -> s_waitcnt lgkmcnt(0) -> the loaded pair is the next address.
// The block is read only; the kernel's one store is the vector store of the last pointer, so the chain stays live.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdint>
#include <cstdlib>
#include <vector>

#define CHECK(call)                                                                                        \
    do {                                                                                                   \
        hipError_t e_ = (call);                                                                            \
        if (e_ != hipSuccess) {                                                                            \
            std::fprintf(stderr, "%s:%d: %s: %s\n", __FILE__, __LINE__, #call, hipGetErrorString(e_));     \
            std::exit(1);                                                                                  \
        }                                                                                                  \
    } while (0)

#define REP 2000
#define UNROLL 16
#define BLOCK_QWORDS 32   // 256 bytes: the size of DevConst

// MODE 0: UNROLL dependent round trips (load, wait, use as the next address)
// MODE 1: groups of four independent loads under ONE wait (what issuing a site's loads together would pay)
// MODE 2: the loop alone (no loads): the overhead to take off
template <int MODE>
__global__ void __launch_bounds__(64) k(const uint64_t* block, uint64_t* out, long long* cyc) {
    uint64_t p = (uint64_t)block, q = p + 8, r = p + 16, s = p + 24;
    const long long t0 = __builtin_readcyclecounter();
    for (int i = 0; i < REP; ++i) {
        if (MODE == 0) {
#pragma unroll
            for (int j = 0; j < UNROLL; ++j)
                asm volatile("s_load_dwordx2 %0, %0, 0x0\n\ts_waitcnt lgkmcnt(0)" : "+s"(p));
        } else if (MODE == 1) {
#pragma unroll
            for (int j = 0; j < UNROLL / 4; ++j)
                asm volatile("s_load_dwordx2 %0, %0, 0x0\n\ts_load_dwordx2 %1, %1, 0x0\n\t"
                             "s_load_dwordx2 %2, %2, 0x0\n\ts_load_dwordx2 %3, %3, 0x0\n\ts_waitcnt lgkmcnt(0)"
                             : "+s"(p), "+s"(q), "+s"(r), "+s"(s));
        } else {
            asm volatile("" : "+s"(p));
        }
    }
    const long long t1 = __builtin_readcyclecounter();
    if (threadIdx.x == 0) {
        out[blockIdx.x] = p ^ q ^ r ^ s;
        cyc[blockIdx.x] = t1 - t0;
    }
}

struct Timing { double ns, counter; };   // one launch: wall time by HIP events, and wave 0's own cycle counter

// base: the same launch with an empty loop body, taken off both figures
template <int MODE>
Timing run(const char* name, int per_rep, int blocks, const uint64_t* block, Timing base) {
    uint64_t* out; long long* cyc;
    CHECK(hipMalloc(&out, sizeof(uint64_t) * blocks));
    CHECK(hipMalloc(&cyc, sizeof(long long) * blocks));
    hipEvent_t e0, e1;
    CHECK(hipEventCreate(&e0)); CHECK(hipEventCreate(&e1));
    hipLaunchKernelGGL(k<MODE>, dim3(blocks), dim3(64), 0, 0, block, out, cyc);   // warm-up
    CHECK(hipGetLastError());
    CHECK(hipEventRecord(e0));
    hipLaunchKernelGGL(k<MODE>, dim3(blocks), dim3(64), 0, 0, block, out, cyc);
    CHECK(hipGetLastError());
    CHECK(hipEventRecord(e1));
    CHECK(hipDeviceSynchronize());
    float ms;
    CHECK(hipEventElapsedTime(&ms, e0, e1));
    std::vector<long long> h(blocks);
    CHECK(hipMemcpy(h.data(), cyc, sizeof(long long) * blocks, hipMemcpyDeviceToHost));
    const Timing t{(double)ms * 1e6, (double)h[0]};
    if (per_rep) {
        const double loads = (double)REP * per_rep, ns = (t.ns - base.ns) / loads;
        std::printf("%-52s blocks=%5d  %.3f ms  -> %.2f ns per load (x2.4 GHz = %.1f cycles)  counter/load %.3f\n", name, blocks, ms,
                    ns, ns * 2.4, (t.counter - base.counter) / loads);
    }
    CHECK(hipEventDestroy(e0)); CHECK(hipEventDestroy(e1));
    CHECK(hipFree(out)); CHECK(hipFree(cyc));
    return t;
}

int main() {
    // qword i holds the address of qword (i * 13 + 5) % 32: one cycle through all 32 (13 = 1 mod 4, 5 odd)
    uint64_t* block;
    CHECK(hipMalloc(&block, sizeof(uint64_t) * BLOCK_QWORDS));
    std::vector<uint64_t> h(BLOCK_QWORDS);
    for (int i = 0; i < BLOCK_QWORDS; ++i) h[i] = (uint64_t)block + 8ull * ((i * 13 + 5) % BLOCK_QWORDS);
    CHECK(hipMemcpy(block, h.data(), sizeof(uint64_t) * BLOCK_QWORDS, hipMemcpyHostToDevice));
    for (int blocks : {256, 1024}) {
        const Timing base = run<2>("", 0, blocks, block, Timing{0.0, 0.0});
        run<0>("16 dependent s_load_dwordx2 + s_waitcnt (round trip)", UNROLL, blocks, block, base);
        run<1>("4 x (4 independent s_load_dwordx2, one s_waitcnt)", UNROLL, blocks, block, base);
    }
    CHECK(hipFree(block));
    return 0;
}
