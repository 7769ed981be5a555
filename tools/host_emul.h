// host_emul.h -- the device vocabulary of cugp_amd/csrc/cov_device.h and append_device.h on a host, for the stand-alone
// checks tools/*_host_check.cpp (no GPU): one workgroup at a time runs as 256 host threads in lock step.  A barrier of
// 256 stands for __syncthreads; a shuffle is an exchange array and two barriers of the caller's own 64-lane wave (waves
// may shuffle different numbers of times between two workgroup barriers, as the corner of k_append_border does).
// __shared__ becomes a function-local static: one copy, shared by the threads of the one workgroup that runs.
// HyperScalars, ExpertPtrs, KERNEL_* and TILE are kernels.h's own -- nothing of the launch interface is declared here.
// A check is: this file, `namespace cugp {` the shared headers `}`, and its main.
#pragma once
#include <barrier>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>

// kernels.h without the HIP runtime: its launcher prototypes need these two names and nothing of them
#define CUGP_HOST_EMUL
typedef struct ihipStream_t* hipStream_t;
typedef struct ihipEvent_t* hipEvent_t;
#include "kernels.h"

typedef double d4 __attribute__((ext_vector_type(4)));
typedef double d2 __attribute__((ext_vector_type(2)));
template <class T> static inline T* GP(T* p) { return p; }

struct Idx { int x = 0, y = 0, z = 0; };
static thread_local Idx threadIdx;
static Idx blockIdx, gridDim;
#define __device__
#define __global__
#define __forceinline__ inline
#define __restrict__
#define __launch_bounds__(...)
#define __shared__ static
#define CUGP_DYN_LDS(name) char* name = nullptr

constexpr int EMUL_THREADS = 256, EMUL_WAVE = 64;
static std::barrier<> g_bar(EMUL_THREADS);
static std::barrier<> g_wbar[EMUL_THREADS / EMUL_WAVE] = {std::barrier<>(EMUL_WAVE), std::barrier<>(EMUL_WAVE),
                                                          std::barrier<>(EMUL_WAVE), std::barrier<>(EMUL_WAVE)};
static double g_slot[EMUL_THREADS];
static inline void __syncthreads() { g_bar.arrive_and_wait(); }
// the value of lane src(lane) of the caller's wave; src < 0: the caller's own
template <class F> static inline double shfl_host(double v, F src)
{
    const int t = threadIdx.x, w = t / EMUL_WAVE, s = src(t % EMUL_WAVE);
    g_slot[t] = v;
    g_wbar[w].arrive_and_wait();
    const double r = s < 0 ? v : g_slot[w * EMUL_WAVE + s];
    g_wbar[w].arrive_and_wait();
    return r;
}
// HIP's rules for a width below the wave: lanes exchange inside their own group of `width`, and a lane whose source lies
// beyond its group keeps its own value
static inline double __shfl_xor(double v, int mask, int width)
{
    return shfl_host(v, [=](int lane) { const int s = lane ^ mask; return s < ((lane + width) & ~(width - 1)) ? s : -1; });
}
static inline double __shfl_down(double v, int delta, int width)
{
    return shfl_host(v, [=](int lane) { return (lane & (width - 1)) + delta < width ? lane + delta : -1; });
}

// f() once per thread of every workgroup, workgroups one after the other (grid: blocks x 1)
template <class F> void launch(int blocks, F f)
{
    gridDim.x = blocks;
    for (int b = 0; b < blocks; b++) {
        blockIdx.x = b;
        std::vector<std::thread> th;
        for (int t = 0; t < EMUL_THREADS; t++) th.emplace_back([=] { threadIdx.x = t; f(); });
        for (auto& x : th) x.join();
    }
}
