/* Definitions for oracle/ref_shim/cuda_runtime.h (host stand-in for the CUDA runtime; test infrastructure). */
#include "cuda_runtime.h"
#include "stb_image_write.h"

thread_local ref_uint3 threadIdx, blockIdx;
thread_local dim3 blockDim, gridDim;

FILE* ref_capture_file = nullptr;

/* Kernels whose result a serial thread loop reproduces exactly; the reasons are in cuda_runtime.h. */
static const char* const SERIAL_EXACT[] = {
    "sumArraysOnGPU",
    "x_derivativeOnGPU", "costVolumOnGPU2",
    "chToFlOnGPU", "flToChOnGPU", "pixelMultOnGPU", "pixelSousOnGPU", "copyFromBigToLittleOnGPU",
    "computeBoxFilterOnGPU", "compute_ak_and_bk", "compute_q", "dispSelectOnGPU",
    "rowSum", "colSum",
    "detect_occlusionOnGPU", "fill_occlusionOnGPU1",
};

void ref_shim_check_kernel(const char* kernel) {
    for (const char* k : SERIAL_EXACT)
        if (!strcmp(k, kernel)) return;
    fprintf(stderr, "ref_shim: kernel %s is not on the list of kernels a serial thread loop runs exactly\n", kernel);
    abort();
}

void ref_capture_q(const float* q, int n) {
    if (ref_capture_file && fwrite(q, sizeof(float), (size_t)n, ref_capture_file) != (size_t)n) {
        fprintf(stderr, "ref_shim: short write of an aggregated plane\n");
        abort();
    }
}

int stbi_write_png(const char*, int w, int h, int comp, const void* data, int) {
    const size_t bytes = (size_t)w * h * comp;
    return ref_capture_file && fwrite(data, 1, bytes, ref_capture_file) == bytes;
}
