// grid_clip.hpp -- the exact clip of one integer Bresenham beam to one tile of the tiled raycast (grid_raycast.hpp), as a plain
// function on values, host and device alike, so that it can be compiled alone: tests/cpp/grid_clip_check.cpp walks the plain
// Bresenham beside it (tests/test_grid_clip.py), at sizes no device test reaches in seconds.  The only device-specific parts
// are the 24-bit product (below) and the reciprocals, which the caller hands in.
//
// A beam runs from (x0, y0) to (x1, y1); u is its major axis (the one with the larger distance du, x on a tie), v the minor
// one (distance dv).  Step i in [0, du] is the cell
//   (u0 + su*i, v0 + sv*floor((2*i*dv + du) / (2*du))),
// the closed form of the walk of oracle/slam_oracle.c (ogrid_raycast): steps 0 .. du-1 are misses, step du is the end cell.
// The steps whose cell lies in a tile are one range [i_lo, i_hi]; the clip finds it with two small integer divisions and
// hands the walk its first cell and the error term there.
#pragma once

#ifdef __HIPCC__
#define SLAM_CLIP_FN __host__ __device__ inline
#else
#define SLAM_CLIP_FN inline
#endif

namespace slam {

SLAM_CLIP_FN int clip_min(int a, int b) { return a < b ? a : b; }
SLAM_CLIP_FN int clip_max(int a, int b) { return a > b ? a : b; }
SLAM_CLIP_FN int clip_abs(int a) { return a < 0 ? -a : a; }

// the low 32 bits of the product of the operands' low 24 bits, taken as signed: __mul24 on the device
SLAM_CLIP_FN int clip_mul24(int a, int b)
{
#ifdef __HIP_DEVICE_COMPILE__
    return __mul24(a, b);
#else
    const int a24 = (int)((unsigned)a << 8) >> 8, b24 = (int)((unsigned)b << 8) >> 8;
    return (int)((unsigned)a24 * (unsigned)b24);
#endif
}

// floor(num / den) for 0 <= num < 2^31, 1 <= den < 2^16, when the quotient is
// below 2^16 (larger quotients saturate to 65536: callers clamp against <= 32767).
// One float multiply + an exact remainder fix instead of an integer division:
// with rden within 1 ulp of 1/den the float quotient is off by < 2^16 * 2^-21,
// so truncation lands on floor or floor +- 1 and the remainder test repairs it.
SLAM_CLIP_FN int floor_div_small(int num, int den, float rden)
{
    const float qf = (float)num * rden;
    if (qf >= 65536.0f) return 65536;
    int       q = (int)qf;
    const int r = (int)((unsigned)num - (unsigned)clip_mul24(q, den));
    q += (r >= den) - (r < 0);
    return q;
}

// the beam's bounding box meets the tile [tx0, tx1] x [ty0, ty1] (what the raycast asks of a whole wavefront before it clips)
SLAM_CLIP_FN bool clip_box_meets_tile(int x0, int y0, int x1, int y1, int tx0, int ty0, int tx1, int ty1)
{
    return clip_max(x0, x1) >= tx0 && clip_min(x0, x1) <= tx1 && clip_max(y0, y1) >= ty0 && clip_min(y0, y1) <= ty1;
}

// den and dv2 of a beam: the caller forms their reciprocals (1 ulp is ample: see floor_div_small)
SLAM_CLIP_FN int clip_den(int x0, int y0, int x1, int y1) { return clip_max(2 * clip_max(clip_abs(x1 - x0), clip_abs(y1 - y0)), 1); }
SLAM_CLIP_FN int clip_dv2(int x0, int y0, int x1, int y1) { return 2 * clip_min(clip_abs(x1 - x0), clip_abs(y1 - y0)); }

struct TileClip {
    int rem;    // steps of the beam inside the tile, 0: none (the other words but den and dv2 are 0 then)
    int a;      // the first of them, step i_lo, as a word of the tile: local y * pitch + local x
    int e;      // the error term (2*i*dv + du) mod 2*du at i_lo, in [0, den)
    int dv2;    // 2*dv: what a step adds to e ...
    int den;    // ... and 2*du (1 for a beam of one cell): where e wraps and the minor axis steps
    int step_u; // what a step adds to a, and what a wrap adds on top
    int step_v;
    int to_end; // du - i_lo: steps from the first one here to the end cell
};

// Coordinates within 0 .. 32767 (beam and tile); rden and rdv2 within one ulp of 1/den and 1/dv2 (rdv2 is not looked at where
// dv2 == 0).  live == false leaves the clip empty: a dropped beam, or the caller's own clip_box_meets_tile.  `pitch`: the
// tile's row pitch in words.  `ablate`: measuring builds switch parts off (wrong counts), everybody else leaves it 0.
SLAM_CLIP_FN TileClip clip_beam_to_tile(int x0, int y0, int x1, int y1, int tx0, int ty0, int tx1, int ty1, int pitch, float rden,
                                        float rdv2, bool live = true, int ablate = 0)
{
    TileClip  c = {0, 0, 0, 0, 1, 0, 0, 0};
    const int dx = clip_abs(x1 - x0), dy = clip_abs(y1 - y0);
    // u = major axis, v = minor axis; step i in [0, du]; i == du is the end cell (hit)
    const bool xm = dx >= dy;
    const int  u0 = xm ? x0 : y0, v0 = xm ? y0 : x0, u1 = xm ? x1 : y1, v1 = xm ? y1 : x1;
    const int  du = xm ? dx : dy, dv = xm ? dy : dx;
    const int  tu0 = xm ? tx0 : ty0, tu1 = xm ? tx1 : ty1;
    const int  tv0 = xm ? ty0 : tx0, tv1 = xm ? ty1 : tx1;
    const bool up = u1 > u0, vp = v1 > v0;
    int        i_lo = clip_max(0, up ? tu0 - u0 : u0 - tu1);
    int        i_hi = clip_min(du, up ? tu1 - u0 : u0 - tu0);
    c.den = clip_max(2 * du, 1);
    c.dv2 = 2 * dv;
    // minor axis: v0 + sv*k in [tv0, tv1]  <=>  k in [k_lo, k_hi]
    const int k_lo = vp ? tv0 - v0 : v0 - tv1;
    const int k_hi = clip_min(vp ? tv1 - v0 : v0 - tv0, dv);
    bool      enters = live && k_hi >= 0 && k_lo <= dv;
    if (enters && dv > 0 && !(ablate & 32)) {
        // k_i >= k_lo  <=>  i >= ceil((2*du*k_lo - du) / (2*dv))
        if (k_lo > 0) i_lo = clip_max(i_lo, floor_div_small(clip_mul24(c.den, k_lo) - du + c.dv2 - 1, c.dv2, rdv2));
        // k_i <= k_hi  <=>  i <= floor((2*du*(k_hi+1) - du - 1) / (2*dv))
        i_hi = clip_min(i_hi, floor_div_small(clip_mul24(c.den, k_hi + 1) - du - 1, c.dv2, rdv2));
    }
    enters = enters && i_lo <= i_hi;
    if (enters && !(ablate & 64)) {
        const int num = clip_mul24(i_lo, c.dv2) + du; // < 2^31
        const int k = du ? floor_div_small(num, c.den, rden) : 0;
        c.e = num - clip_mul24(k, c.den); // running remainder in [0, den)
        const int ul = (up ? u0 + i_lo : u0 - i_lo) - tu0, vl = (vp ? v0 + k : v0 - k) - tv0;
        c.a = xm ? vl * pitch + ul : ul * pitch + vl;
        c.step_u = (up ? 1 : -1) * (xm ? 1 : pitch);
        c.step_v = (vp ? 1 : -1) * (xm ? pitch : 1);
        c.rem = i_hi - i_lo + 1;
        c.to_end = du - i_lo; // steps until the end cell
    }
    return c;
}

} // namespace slam
