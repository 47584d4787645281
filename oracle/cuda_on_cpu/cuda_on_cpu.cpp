/*
 * cuda_on_cpu.cpp -- the fiber scheduler behind cuda_on_cpu.h (test
 * infrastructure only; see the header for the execution model).
 */
#include "cuda_on_cpu.h"

#include <stdlib.h>
#include <sys/mman.h>
#include <ucontext.h>

uint3 threadIdx, blockIdx;
dim3 blockDim, gridDim;

namespace {

const int MAX_THREADS = 1024;              /* CUDA's limit for one block */
const size_t STACK_BYTES = 256 * 1024;     /* per fiber; pages are touched lazily */

int g_descending = 0;
ucontext_t g_scheduler;
ucontext_t g_fiber[MAX_THREADS];
bool g_done[MAX_THREADS];
char *g_stacks = nullptr;
int g_current = -1;
void (*g_body)(void *) = nullptr;
void *g_arg = nullptr;

void fiber_main() {
    g_body(g_arg);
    g_done[g_current] = true;
    /* returning follows uc_link back into the scheduler */
}

uint3 unflatten(long id, dim3 d) {
    uint3 r;
    r.x = (unsigned)(id % d.x);
    r.y = (unsigned)((id / d.x) % d.y);
    r.z = (unsigned)(id / ((long)d.x * d.y));
    return r;
}

}  // namespace

extern "C" void cuda_on_cpu_set_descending(int descending) { g_descending = descending != 0; }

namespace cuda_on_cpu {

void barrier() { swapcontext(&g_fiber[g_current], &g_scheduler); }

void run_grid(dim3 grid, dim3 block, void (*body)(void *), void *arg) {
    const long nthreads = (long)block.x * block.y * block.z;
    const long nblocks = (long)grid.x * grid.y * grid.z;
    if (nthreads < 1 || nthreads > MAX_THREADS || g_current != -1) {
        fprintf(stderr, "cuda_on_cpu: unsupported launch (%ld threads per block)\n", nthreads);
        abort();
    }
    if (!g_stacks) {
        void *p = mmap(nullptr, STACK_BYTES * MAX_THREADS, PROT_READ | PROT_WRITE,
                       MAP_PRIVATE | MAP_ANONYMOUS | MAP_NORESERVE, -1, 0);
        if (p == MAP_FAILED) {
            perror("cuda_on_cpu: mmap");
            abort();
        }
        g_stacks = static_cast<char *>(p);
    }
    gridDim = grid;
    blockDim = block;
    g_body = body;
    g_arg = arg;
    for (long q = 0; q < nblocks; ++q) {
        blockIdx = unflatten(g_descending ? nblocks - 1 - q : q, grid);
        for (long t = 0; t < nthreads; ++t) {
            getcontext(&g_fiber[t]);
            g_fiber[t].uc_stack.ss_sp = g_stacks + STACK_BYTES * t;
            g_fiber[t].uc_stack.ss_size = STACK_BYTES;
            g_fiber[t].uc_link = &g_scheduler;
            makecontext(&g_fiber[t], fiber_main, 0);
            g_done[t] = false;
        }
        long live = nthreads;
        while (live) {
            /* one round: every live fiber runs to its next barrier or to its end */
            for (long s = 0; s < nthreads; ++s) {
                const long t = g_descending ? nthreads - 1 - s : s;
                if (g_done[t]) continue;
                g_current = (int)t;
                threadIdx = unflatten(t, block);
                swapcontext(&g_scheduler, &g_fiber[t]);
                if (g_done[t]) --live;
            }
        }
    }
    g_current = -1;
}

}  // namespace cuda_on_cpu
