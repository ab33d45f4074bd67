// helpers.cuh -- reference stereo_matching_cuda/helpers.cuh:5-6 (exact-equality compare + print), and the float -> 8-bit
// normaliser in front of the PNG writer (the reference keeps its own, write_mat, in main.cu).  Host code only.
#pragma once
#include "SystemIncludes.h"

#include <vector>

bool check_errors(float* resCPU, float* resGPU, int len);
bool check_errors(unsigned char* resCPU, unsigned char* resGPU, int len);

// Float map -> 8-bit image exactly like the reference's write_mat (main.cu:13-35): the maximum is
// the true maximum, but the minimum only considers elements that did NOT raise the running maximum
// at their position (the reference's `else if`); values map through (v - min) * 255 / (max - min)
// in f32 and are truncated.
// Where max == min (a constant map of two or more elements, or one whose elements below the maximum all raised the
// running maximum) the reference divides by zero and converts NaN or an infinity to int, which defines nothing.  Here
// such a map is all zeros, reached without that conversion; smx.write_mat and orc_write_mat_u8 say the same.
inline std::vector<unsigned char> normalise_like_reference(const float* v, size_t n) {
    float hi = -150000000.0f, lo = 150000000.0f;
    for (size_t i = 0; i < n; ++i) {
        const bool raises_max = v[i] > hi;
        if (raises_max) hi = v[i];
        if (!raises_max && v[i] <= lo) lo = v[i];
    }
    std::vector<unsigned char> out(n);
    const float span = hi - lo;
    if (span == 0.0f) return out;
    for (size_t i = 0; i < n; ++i) {
        const int level = (v[i] - lo) * 255.0f / span;
        out[i] = (unsigned char)level;
    }
    return out;
}
