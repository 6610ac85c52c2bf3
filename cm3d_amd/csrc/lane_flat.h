// k_lane_nn_grid (boxes.hip): the index arithmetic of the flat scan.  Plain host/device functions, so that a host program can check them
// against a linear walk (tests/lane_flat_map.cpp).
//
// A step of the ring search leaves every lane of the wave with one range [a, b) of the cell-sorted table (empty for a lane without a
// live segment).  Laid end to end in lane order the ranges are ONE list of T points, and the wave scans that list 64 positions at a
// time: position p belongs to the segment s whose interval [excl(s), incl(s)) of the lengths' prefix sums holds it, and reads
// sorted[a(s) + p - excl(s)] = sorted[p + base(s)] with base(s) = a(s) - excl(s).
#pragma once

#if defined(__HIPCC__)
#define LF_HD __host__ __device__ __forceinline__
#else
#define LF_HD inline
#endif

#define LF_ROUNDS 4                 // rounds of 64 positions whose point loads go out together

// The segment of position p among 64: the smallest s with incl(s) > p, where incl(0..63) are the inclusive prefix sums of the lengths
// (non-decreasing; an empty segment repeats its predecessor's sum and is never the smallest).  Six probes, each at an index below 64;
// p >= incl(63) gives 63.
template <typename Incl>
LF_HD int lf_segment(int p, Incl incl)
{
    int s = 0;
    for (int step = 32; step; step >>= 1)
        if (incl(s + step - 1) <= p) s += step;
    return s;
}

// Five segments (the first ring batch: five rows of the 5 x 5 cells): i0..i3 are the inclusive sums of segments 0..3, v0..v4 the values
// to choose from.  Returns v(s) for the segment s of p; p at or beyond the total gives v4.
LF_HD int lf_pick5(int p, int i0, int i1, int i2, int i3, int v0, int v1, int v2, int v3, int v4)
{
    return p < i0 ? v0 : p < i1 ? v1 : p < i2 ? v2 : p < i3 ? v3 : v4;
}
