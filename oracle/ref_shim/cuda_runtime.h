/*
 * cuda_runtime.h -- host stand-in for the CUDA runtime, used ONLY by oracle/ref_build.py to run a
 * temporary copy of the reference (hamza1030/stereo_matching_cuda) on the CPU.  TEST INFRASTRUCTURE.
 *
 * What it gives: empty qualifiers, dim3, the built-in index variables as thread_local globals,
 * cudaMalloc/cudaMemcpy/cudaFree on the host heap (so a host sanitizer sees every "device" access),
 * and LAUNCH(kernel, grid, block, args...), which ref_build.py puts in place of every
 * `kernel<<<grid, block>>>(args)` of the copy.
 *
 * LAUNCH runs the threads of a grid one after the other.  That is the kernel's own result only when
 * no thread reads what another thread of the same launch writes, or when the result does not depend
 * on the order.  So LAUNCH refuses (abort) every kernel that is not on the list in shim.cpp; the list
 * holds the kernels the five pinned host functions launch, each one read for this property:
 *
 *   rgb_to_grayscale       sumArraysOnGPU                                  own element only
 *   compute_cost           x_derivativeOnGPU, costVolumOnGPU2              read inputs, write own element
 *   compute_guided_filter  chToFlOnGPU, flToChOnGPU, pixelMultOnGPU, pixelSousOnGPU,
 *                          copyFromBigToLittleOnGPU, computeBoxFilterOnGPU, compute_ak_and_bk,
 *                          compute_q, dispSelectOnGPU                      own element only
 *     -> integral          rowSum, colSum     call __syncthreads() inside their loops, but a thread owns
 *                                             a whole row / column: nothing crosses threads, the barrier
 *                                             orders nothing, and a no-op barrier is exact
 *   detect_occlusion       detect_occlusionOnGPU   writes own element of the left map, reads the right map
 *   fill_occlusion         fill_occlusionOnGPU1    reads and writes one map in place; the result is the
 *                                                  same for every order (oracle/REF_CASES.md)
 *
 * No kernel on the list declares __shared__ memory.  The kernels that do (transpose, rowSum_sm, the
 * tile kernels of filter.cu) need a real barrier; they are not on the list, filter.cu is not even
 * compiled, and nothing is pinned through them.
 */
#pragma once
#include <cstdio>
#include <cstdlib>
#include <cstring>

#define __host__
#define __device__
#define __global__
#define __shared__ static

struct ref_uint3 { unsigned x, y, z; };
struct dim3 {
    unsigned x, y, z;
    dim3(unsigned a = 1, unsigned b = 1, unsigned c = 1) : x(a), y(b), z(c) {}
};
extern thread_local ref_uint3 threadIdx, blockIdx;
extern thread_local dim3 blockDim, gridDim;

/* only rowSum / colSum get here (see above) */
inline void __syncthreads() {}

typedef int cudaError_t;
enum { cudaSuccess = 0 };
enum cudaMemcpyKind { cudaMemcpyHostToDevice, cudaMemcpyDeviceToHost, cudaMemcpyDeviceToDevice };
struct cudaDeviceProp { char name[64]; };

template <class T> inline cudaError_t cudaMalloc(T** p, size_t bytes) { *p = (T*)malloc(bytes); return cudaSuccess; }
inline cudaError_t cudaFree(void* p) { free(p); return cudaSuccess; }
inline cudaError_t cudaMemcpy(void* d, const void* s, size_t bytes, cudaMemcpyKind) { memcpy(d, s, bytes); return cudaSuccess; }
inline cudaError_t cudaMemset(void* d, int v, size_t bytes) { memset(d, v, bytes); return cudaSuccess; }
inline cudaError_t cudaDeviceSynchronize() { return cudaSuccess; }
inline cudaError_t cudaGetLastError() { return cudaSuccess; }
inline cudaError_t cudaSetDevice(int) { return cudaSuccess; }
inline cudaError_t cudaDeviceReset() { return cudaSuccess; }
inline cudaError_t cudaGetDeviceProperties(cudaDeviceProp* p, int) { strcpy(p->name, "host"); return cudaSuccess; }
inline const char* cudaGetErrorString(cudaError_t) { return "host stand-in"; }

/* aborts unless `kernel` is on the list of kernels a serial thread loop runs exactly (shim.cpp) */
void ref_shim_check_kernel(const char* kernel);

/* ref_build.py adds a call after compute_q in the copy of guidedFilter.cu: appends the slice's aggregated
 * plane to ref_capture_file when the driver has opened one (the reference never keeps the volume) */
extern FILE* ref_capture_file;
void ref_capture_q(const float* q, int n);

/* `::` on purpose: host functions of the reference declare locals named blockDim / gridDim */
#define LAUNCH(k, G, B, ...)                                                              \
    do {                                                                                  \
        ref_shim_check_kernel(#k);                                                        \
        const dim3 g_ = (G), b_ = (B);                                                    \
        ::blockDim = b_;                                                                  \
        ::gridDim = g_;                                                                   \
        for (unsigned bz_ = 0; bz_ < g_.z; ++bz_)                                         \
        for (unsigned by_ = 0; by_ < g_.y; ++by_)                                         \
        for (unsigned bx_ = 0; bx_ < g_.x; ++bx_)                                         \
        for (unsigned tz_ = 0; tz_ < b_.z; ++tz_)                                         \
        for (unsigned ty_ = 0; ty_ < b_.y; ++ty_)                                         \
        for (unsigned tx_ = 0; tx_ < b_.x; ++tx_) {                                       \
            ::blockIdx = {bx_, by_, bz_};                                                 \
            ::threadIdx = {tx_, ty_, tz_};                                                \
            k(__VA_ARGS__);                                                               \
        }                                                                                 \
    } while (0)
