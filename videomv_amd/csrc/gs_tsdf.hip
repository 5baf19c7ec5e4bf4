// gfx950 (MI355X) — TSDF fusion of the orbit's median-depth maps into a voxel volume (videomv_amd/gs_mesh.py; contract in
// include/vmv.h, "TSDF fusion").  All fp32.
//   gs_tsdf_integrate_kernel   one thread per voxel, 256-thread blocks over the linear voxel index (x fastest: a wave's lanes are 64
//                              neighbouring voxels of one x row, or the end of one and the start of the next, and project to neighbouring
//                              pixels); the thread walks the views in index order with its seven accumulators in registers: one read and
//                              one write per plane per call, no atomics, a deterministic function of the inputs.
// The camera rows are indexed by the loop counter alone (wave-uniform: scalar loads).  Views go in batches of four: first the four
// projections and their depth gathers, each issued at a pixel clamped into the image whether or not the view will count, then the
// definition's branches over the four values in view order — four independent gathers in flight per thread instead of one behind a
// branch (written as one loop the compiler moved the load under the visibility test and waited for it there).  The colour gather
// stays behind its branch: only voxels inside the truncation band take it.  Projection and pixel mapping: gs_mesh_common.h.
#include "gs_mesh_common.h"

namespace {

constexpr int TS_BATCH = 4;                     // views per batch: depth gathers in flight per thread

struct TsdfGeom {
    int n_views, size, res, carve;
    float tan_half_fov, ox, oy, oz, voxel, trunc, z_min;
};

__global__ __launch_bounds__(256) void gs_tsdf_integrate_kernel(const float* __restrict__ depth, const float* __restrict__ colour,
                                                                const float* __restrict__ views, const TsdfGeom g, float* __restrict__ acc,
                                                                const size_t plane_stride) {
    const unsigned R = (unsigned)g.res;
    // blocks are dealt round-robin to the 8 XCDs: give each XCD a contiguous slab of the volume (gemm_common.h), so that the voxel rows
    // it works on at one time are neighbours and find each other's depth-map lines in its L2
    const unsigned blk = (unsigned)vmvg::xcd_logical((int)blockIdx.x, (int)gridDim.x);
    const unsigned idx = blk * 256u + threadIdx.x;                     // R <= 1024: R^3 + 255 < 2^32
    if (idx >= R * R * R) return;
    const unsigned ix0 = idx % R, t = idx / R;
    const unsigned iy0 = t % R, iz0 = t / R;
    const float wx = g.ox + (float)ix0 * g.voxel, wy = g.oy + (float)iy0 * g.voxel, wz = g.oz + (float)iz0 * g.voxel;
    float* const a0 = acc + idx;
    float s_tsdf = a0[0], s_w = a0[plane_stride], s_behind = a0[2 * plane_stride];
    float s_r = 0.f, s_g = 0.f, s_b = 0.f, s_wc = 0.f;
    if (colour) {
        s_r = a0[3 * plane_stride];
        s_g = a0[4 * plane_stride];
        s_b = a0[5 * plane_stride];
        s_wc = a0[6 * plane_stride];
    }
    const float fS = (float)g.size, hi = (float)(g.size - 1);
    const size_t S = (size_t)g.size, SS = S * S;
    for (int v0 = 0; v0 < g.n_views; v0 += TS_BATCH) {
        // phase 1: project into TS_BATCH views and issue their depth gathers, every one at a pixel clamped into the image
        float zc[TS_BATCH], dd[TS_BATCH];
        unsigned po[TS_BATCH];                                         // pixel offset inside a view: size <= 32768, so size^2 <= 2^30
        bool seen[TS_BATCH];
#pragma unroll
        for (int j = 0; j < TS_BATCH; ++j) {
            const int v = min(v0 + j, g.n_views - 1);                  // past the last view: that view again, masked out below
            const auto [xv, yv, z] = mesh_project(views + 16 * (size_t)v, wx, wy, wz);
            const float inv = 1.0f / (z * g.tan_half_fov);
            const float fx = mesh_nearest(mesh_pixel(xv, inv, fS)), fy = mesh_nearest(mesh_pixel(yv, inv, fS));
            // the range test on the floats (a voxel near the camera plane gives an enormous or a NaN pixel); false for NaN
            seen[j] = v0 + j < g.n_views && z > g.z_min && fx >= 0.0f && fx < fS && fy >= 0.0f && fy < fS;
            // fmaxf / fminf return the other operand for a NaN: the clamped pixel is always inside the image
            po[j] = (unsigned)fminf(fmaxf(fy, 0.0f), hi) * (unsigned)g.size + (unsigned)fminf(fmaxf(fx, 0.0f), hi);
            zc[j] = z;
            dd[j] = depth[(size_t)v * SS + po[j]];
        }
        // phase 2: the definition's branches, in view order; a view that does not count reads as d = -1: no branch takes it
#pragma unroll
        for (int j = 0; j < TS_BATCH; ++j) {
            const float d = seen[j] ? dd[j] : -1.0f;
            if (d > 0.0f) {
                const float sdf = d - zc[j];
                if (sdf < -g.trunc) {
                    s_behind += 1.0f;                                  // hidden behind the surface
                } else {
                    s_tsdf += fminf(1.0f, sdf / g.trunc);
                    s_w += 1.0f;
                    if (colour && sdf <= g.trunc) {
                        const float* __restrict__ c = colour + (size_t)(v0 + j) * 3 * SS + po[j];
                        s_r += c[0];
                        s_g += c[SS];
                        s_b += c[2 * SS];
                        s_wc += 1.0f;
                    }
                }
            } else if (d == 0.0f && g.carve) {
                s_tsdf += 1.0f;                                        // the ray reached no surface: free space
                s_w += 1.0f;
            }
        }
    }
    a0[0] = s_tsdf;
    a0[plane_stride] = s_w;
    a0[2 * plane_stride] = s_behind;
    if (colour) {
        a0[3 * plane_stride] = s_r;
        a0[4 * plane_stride] = s_g;
        a0[5 * plane_stride] = s_b;
        a0[6 * plane_stride] = s_wc;
    }
}

}  // namespace

extern "C" int vmv_gs_tsdf_integrate(const VmvGsTsdfParams* pp, void* stream) {
    if (!pp) return VMV_ENULL;
    const VmvGsTsdfParams& p = *pp;
    if (!p.depth || !p.views || !p.acc) return VMV_ENULL;
    if (p.n_views < 1 || p.size < 1 || p.res < 2 || p.res > 1024) return VMV_EINVAL;
    if (p.size > MESH_MAX_VIEW_SIZE) return VMV_ERANGE;                // this entry point refuses the size before the values, as it always has
    const int ev = mesh_check_views(p.depth, p.colour, p.views, p.n_views, p.size, p.tan_half_fov, p.z_min);
    if (ev == VMV_EINVAL || !(p.voxel > 0.f) || !(p.trunc > 0.f)) return VMV_EINVAL;
    const long n = (long)p.res * p.res * p.res;
    if (p.plane_stride < n) return VMV_EINVAL;
    if (ev || ((uintptr_t)p.acc & 3)) return ev ? ev : VMV_EALIGN;
    const TsdfGeom g{p.n_views, p.size, p.res, p.carve ? 1 : 0, p.tan_half_fov, p.origin[0], p.origin[1], p.origin[2], p.voxel, p.trunc, p.z_min};
    hipLaunchKernelGGL(gs_tsdf_integrate_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                       p.depth, p.colour, p.views, g, p.acc, (size_t)p.plane_stride);
    return vmv_launch_status();
}
