// gfx950 kernel of vj_track: for every row the t x t gray template T and the (t + 2 r)^2 search patch S that
// vj_extract's kernel wrote into scratch, matched at the (2 r + 1)^2 displacements:
//   track_match    sad(dx, dy) = sum |T[i][j] - S[i + r + dy][j + r + dx]|, the smallest (sad, dx^2 + dy^2, dy, dx), and sad(0, 0)
// Integers only.  One workgroup (4 waves) per row.  T and S go from scratch into LDS with dword loads: T dense (t is a multiple
// of 4), S with its rows padded to whole dwords — t + 2 r is even, so every other row of a patch whose side is no multiple of 4
// starts 2 bytes into a dword: there two loads and v_alignbyte bring it to phase 0, everywhere else it is one load.  At most
// 4096 + 9232 bytes.  The index arithmetic is vj_track_units.hpp's, which tests/track_asan_driver.cpp walks on the CPU.
//
// The displacements are dealt over the lanes in units of four neighbouring dx of one dy: unit (dy, u) owns dx + r = 4 u .. 4 u + 3,
// the ones above 2 r are computed and left out.  For four template pixels T[i][4 q .. 4 q + 3] (one dword, the same LDS address in
// every lane: a broadcast) the unit needs the eight bytes of S's row i + r + dy from column 4 u + 4 q on: two neighbouring
// dwords, of which one was the last step's, so ONE ds_read_b32 per lane and step, and ONE v_qsad_pk_u16_u8, which adds the four
// SADs of the dword against the four byte phases of the 8-byte window to four packed u16 accumulators.  Those hold 65535:
// they are flushed into 32-bit sums every four template rows, at most 4 * 64 = 256 pixels of difference 255 = 65280.
// (v_mqsad_* is not usable: it skips reference bytes that are 0.)
//
// The best tuple is the minimum of the 64-bit key sad << 32 | (dx^2 + dy^2) << 16 | (dy + r) << 8 | (dx + r): per lane, per wave
// (shuffles), across the waves through LDS; lane 0 writes the 16-byte record with one vector store.
#include <hip/hip_runtime.h>
#include "vj_track_units.hpp"
#include "vj_devutil.hpp"

namespace vj {

// Every global load lies inside the row's template (t * t bytes) or its search patch ((t + 2 r)^2 bytes: the dword index is clamped
// to the patch's last), every LDS index below the arrays' sizes (a window reads at most one dword past its row: the next row's
// first, or the pad behind the last row), the one global store inside out[first + n).
__global__ __launch_bounds__(TRACK_THREADS) void track_match(TrackArgs a) {
    __shared__ uint32_t Tl[TRACK_T_DWORDS];
    __shared__ uint32_t Sl[TRACK_S_DWORDS];
    __shared__ unsigned long long best_l[TRACK_THREADS / 64u];
    __shared__ uint32_t sad0_l;
    if (blockIdx.x >= a.n) return;   // (uniform)
    const uint32_t row = a.first + blockIdx.x, tid = threadIdx.x;
    const TrackGeom g = track_geom(a.t, a.r);
    const uint32_t* Tg = reinterpret_cast<const uint32_t*>(a.tmpl + (size_t)row * g.t * g.t);
    const uint32_t* Sg = reinterpret_cast<const uint32_t*>(a.search + (size_t)row * a.search_pitch);
    for (uint32_t i = tid; i < g.n_t; i += TRACK_THREADS) Tl[i] = Tg[i];
    for (uint32_t i = tid; i < g.n_sl + TRACK_S_PAD; i += TRACK_THREADS) {
        uint32_t v = 0;
        if (i < g.n_sl) {
            const TrackFill f = track_fill(g, i);
            v = Sg[f.lo];
            if (f.phase != 0u) v = __builtin_amdgcn_alignbyte(Sg[f.hi], v, f.phase);
        }
        Sl[i] = v;
    }
    __syncthreads();

    unsigned long long best = ~0ull;
    for (uint32_t unit = tid; unit < g.n_units; unit += TRACK_THREADS) {
        uint32_t dyi, u;
        track_unit(g, unit, &dyi, &u);
        uint32_t sum[4] = {0u, 0u, 0u, 0u};
        for (uint32_t i = 0; i < g.t; i += 4u) {
            unsigned long acc = 0;
#pragma unroll
            for (uint32_t ii = 0; ii < 4u; ++ii) {
                const uint32_t sb = track_s_base(g, i + ii, dyi, u), tb = track_t_base(g, i + ii);
                uint32_t w0 = Sl[sb];
                for (uint32_t q = 0; q < g.td; ++q) {
                    const uint32_t w1 = Sl[sb + q + 1u], tw = Tl[tb + q];
                    acc = __builtin_amdgcn_qsad_pk_u16_u8(((unsigned long)w1 << 32) | w0, tw, acc);
                    w0 = w1;
                }
            }
            sum[0] += (uint32_t)(acc & 0xffffu);
            sum[1] += (uint32_t)((acc >> 16) & 0xffffu);
            sum[2] += (uint32_t)((acc >> 32) & 0xffffu);
            sum[3] += (uint32_t)(acc >> 48);
        }
#pragma unroll
        for (uint32_t q = 0; q < 4u; ++q) {
            const uint32_t dxi = 4u * u + q;
            if (dxi >= g.side) continue;
            const unsigned long long key = track_key(g, sum[q], dyi, dxi);
            best = key < best ? key : best;
            if (dxi == g.r && dyi == g.r) sad0_l = sum[q];   // one lane of the workgroup
        }
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const unsigned long long o = __shfl_xor(best, m, 64);
        best = o < best ? o : best;
    }
    if ((tid & 63u) == 0u) best_l[tid >> 6] = best;
    __syncthreads();
    if (tid == 0u) {
#pragma unroll
        for (uint32_t w = 1; w < TRACK_THREADS / 64u; ++w) best = best_l[w] < best ? best_l[w] : best;
        const int32_t dx = (int32_t)(best & 0xffu) - (int32_t)g.r, dy = (int32_t)((best >> 8) & 0xffu) - (int32_t)g.r;
        *reinterpret_cast<int4*>(a.out + row) = make_int4(dx, dy, (int32_t)(uint32_t)(best >> 32), (int32_t)sad0_l);
    }
}

int launch_track(const TrackArgs& a, void* stream_) {
    if (a.n == 0u) return 0;
    if (a.t < TRACK_TMPL_MIN || a.t > TRACK_TMPL_MAX || (a.t & 3u) != 0u || a.r < TRACK_RADIUS_MIN || a.r > TRACK_RADIUS_MAX ||
        (a.search_pitch & 15u) != 0u || a.search_pitch < (uint64_t)(a.t + 2u * a.r) * (a.t + 2u * a.r))
        return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(track_match, dim3(a.n), dim3(TRACK_THREADS), 0, (hipStream_t)stream_, a);
    return (int)hipGetLastError();
}

}  // namespace vj
