/*
 * cuda_on_cpu.h -- just enough of the CUDA programming model to run a plain
 * CUDA kernel file on the host, for PINNING THE ORACLE ONLY (oracle/ref_build.py).
 *
 * TEST INFRASTRUCTURE ONLY.  Nothing in the product path includes this file.
 *
 * Model:
 *   - one OS thread; the blocks of a grid run one after the other;
 *   - the threads of one block are ucontext fibers that yield at
 *     __syncthreads().  The scheduler resumes every live fiber once per round,
 *     so a round ends exactly when each fiber has reached its next barrier or
 *     returned; a fiber that has returned counts as arrived at every later one;
 *   - blocks (by linear id x + gridDim.x * (y + gridDim.y * z)) and the threads
 *     inside a block run in ASCENDING order, or in DESCENDING order after
 *     cuda_on_cpu_set_descending(1).  Between two barriers every fiber runs to
 *     completion before the next one starts, so among racing plain stores the
 *     last fiber in schedule order wins: under the descending schedule that is
 *     the LOWEST index;
 *   - __shared__ is a function-local static (one block at a time, so one copy);
 *   - atomics are plain read-modify-writes.
 *
 * A kernel launch `k<<<grid, block>>>(args)` is not C++.  ref_build.py rewrites
 * it textually into `CUDA_ON_CPU_LAUNCH(k, grid, block)(args)` in a scratch copy
 * of the source before compiling it.
 *
 * Do not build this with a sanitizer: ASan does not follow swapcontext().
 */
#ifndef PCM_CUDA_ON_CPU_H
#define PCM_CUDA_ON_CPU_H

#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#define __global__
#define __device__
#define __host__
#define __forceinline__ inline __attribute__((always_inline))
#define __shared__ static

struct uint3 {
    unsigned x, y, z;
};
struct dim3 {
    unsigned x, y, z;
    dim3(unsigned long long x_ = 1, unsigned long long y_ = 1, unsigned long long z_ = 1)
        : x((unsigned)x_), y((unsigned)y_), z((unsigned)z_) {}
};
extern uint3 threadIdx, blockIdx;
extern dim3 blockDim, gridDim;

extern "C" void cuda_on_cpu_set_descending(int descending);

namespace cuda_on_cpu {

void barrier();
/* runs body(arg) once per thread of the grid, under the current schedule */
void run_grid(dim3 grid, dim3 block, void (*body)(void *), void *arg);

struct LaunchConfig {
    dim3 grid, block;
    LaunchConfig(dim3 g, dim3 b, size_t /*dynamic shared bytes*/ = 0, void * /*stream*/ = nullptr)
        : grid(g), block(b) {}
};

template <class... P>
struct BoundKernel {
    void (*kernel)(P...);
    LaunchConfig cfg;
    /* the arguments are evaluated once, by the caller, and converted to the
     * kernel's parameter types once, as a real launch does */
    void operator()(P... args) const {
        auto body = [&]() { kernel(args...); };
        run_grid(cfg.grid, cfg.block, [](void *p) { (*static_cast<decltype(body) *>(p))(); }, &body);
    }
};

template <class... P>
BoundKernel<P...> bind(void (*kernel)(P...), LaunchConfig cfg) {
    return BoundKernel<P...>{kernel, cfg};
}

}  // namespace cuda_on_cpu

#define __syncthreads() cuda_on_cpu::barrier()
#define CUDA_ON_CPU_LAUNCH(kernel, ...) cuda_on_cpu::bind(kernel, cuda_on_cpu::LaunchConfig(__VA_ARGS__))

/* device intrinsics and atomics the kernels use (single OS thread: plain RMW) */
static inline int __float_as_int(float f) { int i; memcpy(&i, &f, sizeof i); return i; }
static inline float __int_as_float(int i) { float f; memcpy(&f, &i, sizeof f); return f; }
static inline int atomicCAS(int *a, int expect, int v) { int old = *a; if (old == expect) *a = v; return old; }
static inline int atomicAdd(int *a, int v) { int old = *a; *a = old + v; return old; }
static inline float atomicAdd(float *a, float v) { float old = *a; *a = old + v; return old; }
static inline int min(int a, int b) { return a < b ? a : b; }
static inline int max(int a, int b) { return a > b ? a : b; }
/* CUDA's float min/max return the non-NaN operand, as fminf/fmaxf do */
static inline float min(float a, float b) { return fminf(a, b); }
static inline float max(float a, float b) { return fmaxf(a, b); }

/* the few runtime calls the host functions make; nothing here can fail */
typedef int cudaError_t;
enum { cudaSuccess = 0 };
static inline cudaError_t cudaGetLastError() { return cudaSuccess; }
static inline const char *cudaGetErrorString(cudaError_t) { return "no error"; }

/* at::Tensor as the host functions use it: sizes and a typed data pointer */
namespace at {
struct Tensor {
    void *ptr;
    int64_t sizes[3];
    int64_t size(int i) const { return sizes[i]; }
    template <class T>
    T *data() const { return static_cast<T *>(ptr); }
};
}  // namespace at

#endif
