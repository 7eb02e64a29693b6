// Index arithmetic of the max-pool and of its gradient as a gather (csrc/pool_train.hip).  A pool of kernel k, stride s and padding
// pad (pad < k, s >= 1) maps `in` pixels of an axis to out = (in + 2 pad - k) / s + 1 windows; window o covers the positions
// o * s - pad + t for the taps t = 0 ... k - 1, of which those in [0, in) exist (the window is CUT at the border, not clamped).
// The forward stores per output element the tap index ty * k + tx of the position that gave the maximum; the backward lets every
// input pixel visit the windows that cover it -- a contiguous range [pa_first, pa_last] per axis, possibly empty -- and asks each
// whether its stored tap is the tap this pixel is in that window.  With s >= k - 1 at most two windows per axis cover a pixel.
// Integer arithmetic only; compiles for the device and for the host (tests/pool_adjoint_host.cpp runs it against brute force under
// sanitizers).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PA_HD __host__ __device__ __forceinline__
#else
#define PA_HD inline
#endif

// windows along an axis of `in` pixels (0: the axis is shorter than a window, padding included)
PA_HD int pa_out(int in, int k, int s, int pad) { return in + 2 * pad < k ? 0 : (in + 2 * pad - k) / s + 1; }

// the first window that covers pixel i: the smallest o >= 0 with o * s - pad + k - 1 >= i
PA_HD int pa_first(int i, int k, int s, int pad) {
    const int a = i + pad - k + 1;
    return a <= 0 ? 0 : (a + s - 1) / s;
}

// the last window that covers pixel i: the largest o <= out - 1 with o * s - pad <= i (below pa_first: no window covers i)
PA_HD int pa_last(int i, int s, int pad, int out) {
    const int b = (i + pad) / s;
    return b < out - 1 ? b : out - 1;
}

// the tap pixel i is in window o (0 ... k - 1 for a window that covers it), and the position of tap t of window o
PA_HD int pa_tap(int i, int o, int s, int pad) { return i - (o * s - pad); }
PA_HD int pa_position(int o, int t, int s, int pad) { return o * s - pad + t; }

// the stored index of tap (ty, tx) and its two parts
PA_HD int pa_index(int ty, int tx, int k) { return ty * k + tx; }
PA_HD int pa_index_ty(int index, int k) { return index / k; }
PA_HD int pa_index_tx(int index, int k) { return index % k; }
