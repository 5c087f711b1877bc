// Records and index arithmetic the match kernel (vj_track.hip) shares with the host code that launches it
// (vj_track.cpp), lays its scratch out (vj_track_host.cpp, which is compiled without HIP for the sanitizer runs) and walks its
// indices under the sanitizers (tests/track_asan_driver.cpp): plain PODs and inline functions, nothing else.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define VJ_TRACK_HD __host__ __device__
#else
#define VJ_TRACK_HD
#endif

namespace vj {

constexpr uint32_t TRACK_TMPL_MIN = 8, TRACK_TMPL_MAX = 64, TRACK_RADIUS_MIN = 1, TRACK_RADIUS_MAX = 16;
constexpr uint32_t TRACK_SEARCH_MAX = TRACK_TMPL_MAX + 2u * TRACK_RADIUS_MAX;   // 96: the side of the largest search patch

// The kernel's workgroup and its two LDS arrays, in dwords: T dense, S with its rows padded to whole dwords, plus the pad a
// window reads behind the last row.
constexpr uint32_t TRACK_THREADS = 256;
constexpr uint32_t TRACK_T_DWORDS = TRACK_TMPL_MAX * TRACK_TMPL_MAX / 4u;             // 1024
constexpr uint32_t TRACK_S_PAD = 4;
constexpr uint32_t TRACK_S_DWORDS = TRACK_SEARCH_MAX * (TRACK_SEARCH_MAX / 4u) + TRACK_S_PAD;   // 2304 + 4

// The geometry of one (t, r): everything the kernel indexes with.
struct TrackGeom {
    uint32_t t, r;
    uint32_t P;         // t + 2 r: the side of the search patch
    uint32_t Pd;        // dwords of a row of S in LDS: P rounded up to 4, over 4
    uint32_t td;        // dwords of a row of T: t / 4
    uint32_t n_t;       // dwords of T, in scratch and in LDS
    uint32_t n_s;       // dwords of S in scratch: P * P / 4 (P is even)
    uint32_t n_sl;      // dwords of S in LDS without the pad: P * Pd
    uint32_t side;      // 2 r + 1 displacements per axis
    uint32_t U;         // units of four neighbouring dx per dy
    uint32_t n_units;   // side * U
};
VJ_TRACK_HD inline TrackGeom track_geom(uint32_t t, uint32_t r) {
    TrackGeom g;
    g.t = t;
    g.r = r;
    g.P = t + 2u * r;
    g.Pd = (g.P + 3u) >> 2;
    g.td = t >> 2;
    g.n_t = g.td * t;
    g.n_s = (g.P * g.P) >> 2;
    g.n_sl = g.P * g.Pd;
    g.side = 2u * r + 1u;
    g.U = (g.side + 3u) >> 2;
    g.n_units = g.side * g.U;
    return g;
}

// LDS dword i < n_sl of S holds bytes 4 q .. 4 q + 3 of row y: they begin at byte `off` of the dense patch in scratch, in dword
// `lo` at byte phase `phase` (0, or 2 in every other row of a patch whose side is no multiple of 4); `hi` is the dword that holds
// the rest, looked at only when phase != 0.  Both are clamped to the patch's last dword.
struct TrackFill { uint32_t lo, hi, phase; };
VJ_TRACK_HD inline TrackFill track_fill(const TrackGeom& g, uint32_t i) {
    const uint32_t y = i / g.Pd, q = i - y * g.Pd, off = y * g.P + 4u * q, d = off >> 2, last = g.n_s - 1u;
    TrackFill f;
    f.lo = d < last ? d : last;
    f.hi = d + 1u < last ? d + 1u : last;
    f.phase = off & 3u;
    return f;
}

// Unit `unit` < n_units: its dy + r and the first of its four dx + r.
VJ_TRACK_HD inline void track_unit(const TrackGeom& g, uint32_t unit, uint32_t* dyi, uint32_t* u) {
    *dyi = unit / g.U;
    *u = unit - *dyi * g.U;
}
// The first LDS dword of S a unit reads for template row i (it reads td + 1 dwords from there on), and of T.
VJ_TRACK_HD inline uint32_t track_s_base(const TrackGeom& g, uint32_t i, uint32_t dyi, uint32_t u) { return (i + dyi) * g.Pd + u; }
VJ_TRACK_HD inline uint32_t track_t_base(const TrackGeom& g, uint32_t i) { return i * g.td; }
// The 64-bit key whose minimum is the best tuple (sad, dx^2 + dy^2, dy, dx).
VJ_TRACK_HD inline uint64_t track_key(const TrackGeom& g, uint32_t sad, uint32_t dyi, uint32_t dxi) {
    const int32_t dx = (int32_t)dxi - (int32_t)g.r, dy = (int32_t)dyi - (int32_t)g.r;
    return ((uint64_t)sad << 32) | ((uint64_t)(uint32_t)(dx * dx + dy * dy) << 16) | (uint64_t)(dyi << 8) | dxi;
}

// What the kernel writes per row; the host adds the box (step 5 of the definition is f64 arithmetic on the mapped regions).
struct TrackMatchDev {
    int32_t  dx, dy;
    uint32_t sad, sad0;
};
static_assert(sizeof(TrackMatchDev) == 16, "TrackMatchDev is 16 bytes");

// Row k's template is the t * t bytes at tmpl + k * t * t, its search patch the (t + 2 r)^2 bytes at search + k * search_pitch, rows
// dense; both addresses and both pitches are multiples of 16.  Rows [first, first + n) are matched, one workgroup each.
struct TrackArgs {
    const uint8_t* tmpl;
    const uint8_t* search;
    TrackMatchDev* out;
    uint64_t search_pitch;
    uint32_t first, n;
    uint32_t t, r;
};
int launch_track(const TrackArgs& a, void* stream);

}  // namespace vj
