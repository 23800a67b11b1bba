// table_launch.hpp -- what the launchers that carry a TABLE of caller entries as kernel arguments share (adam.hip, smoothness.hip,
// packing.hip, pack_image.hip), host code only: pad_table, which fills the fixed-size argument array; the exact test that nothing a
// launch writes lies on anything else it touches (Interval, add_planes, written_overlaps); and whole_quads, the divisibility half of a
// quad-path test.  Which pointers of an entry are read and which are written is each launcher's own.
#pragma once
#include <algorithm>
#include <vector>

#include "launch_util.hpp"

namespace pbr {

// The N slots of a kernel-argument array from the caller's n entries (1 <= n <= N, checked by the entry point): entry 0 is repeated
// behind them, so every slot holds a valid entry whatever the kernel reads.
template <typename T, size_t N> inline void pad_table(T (&dst)[N], const T *src, int32_t n) {
    for (size_t i = 0; i < N; ++i) dst[i] = src[i < (size_t)n ? i : 0];
}

// Every value divisible by 4: a width or pixel count and the strides of an entry whose planes are to be walked in quads.
inline bool whole_quads(std::initializer_list<int64_t> values) {
    return std::all_of(values.begin(), values.end(), [](int64_t v) { return v % 4 == 0; });
}

// [lo, hi): bytes a launch touches without a gap, and whether it writes them.
struct Interval { uintptr_t lo, hi; bool written; };

// The intervals of [batch] x [channels] dense planes of `pixels` elements of `esz` bytes at the given strides (in elements): one per
// plane, per image where an image's planes are back to back, one in all where the images are too.  The views of a material-major packing
// interleave the maps of a batch -- material 0's normal lies between material 0's and material 1's albedo -- so a pointer's first-to-last
// span says nothing there.
inline void add_planes(std::vector<Interval> &out, const void *p, int32_t batch, int32_t channels, int64_t pixels, int64_t batch_stride,
                       int64_t plane_stride, size_t esz, bool written) {
    const uintptr_t base = reinterpret_cast<uintptr_t>(p);
    const bool image_dense = channels == 1 || plane_stride == pixels;
    const bool all_dense = image_dense && (batch == 1 || batch_stride == (int64_t)channels * pixels);
    const int32_t images = all_dense ? 1 : batch, planes = image_dense ? 1 : channels;         // the runs, each of `run` elements
    const int64_t run = (int64_t)(batch / images) * (channels / planes) * pixels;
    for (int32_t b = 0; b < images; ++b) {
        for (int32_t c = 0; c < planes; ++c) {
            const uintptr_t lo = base + (uintptr_t)((int64_t)b * batch_stride + (int64_t)c * plane_stride) * esz;
            out.push_back({lo, lo + (uintptr_t)run * esz, written});
        }
    }
}

// Nothing that is written may overlap anything else the launch touches; what is only read -- a gradient that is an input, an expanded
// tensor's repeated planes -- may overlap itself.  Exact for strided entries: every interval is a run the kernel really touches, and
// intervals that merely touch do not overlap.  Sorts `iv`.
inline bool written_overlaps(std::vector<Interval> &iv) {
    std::sort(iv.begin(), iv.end(), [](const Interval &a, const Interval &b) { return a.lo < b.lo; });
    uintptr_t end_written = 0, end_any = 0;                             // the furthest end among the intervals in front
    for (const Interval &x : iv) {
        if (x.lo < end_written || (x.written && x.lo < end_any)) return true;
        if (x.written && x.hi > end_written) end_written = x.hi;
        if (x.hi > end_any) end_any = x.hi;
    }
    return false;
}

}  // namespace pbr
