// gfx950 (MI355X) — texture baking: the orbit views' colours blended over a triangle mesh into a texture atlas (videomv_amd/gs_mesh.py:
// bake_texture; contract in include/vmv.h, "Texture baking").  All fp32, plain loads and stores.
//   bake_clear_kernel   one thread: *status = 0
//   gs_mesh_bake_kernel one thread per texel, 256-thread blocks over the texels in CELL order: thread index = cell * P^2 + j * P + i, so a
//                       wave's 64 lanes are one 8 x 8 cell at the default patch (four cells at P = 4; cells straddle waves where P^2 is no
//                       multiple of 64).  The lanes of a cell share two faces — the index and vertex loads of a wave fall into a few
//                       cache lines — and project to a patch of neighbouring pixels of every view; a store instruction writes P-texel
//                       runs of P rows.  Measured against the flat order (thread index = y * T + x: whole-line stores, 16 faces per
//                       wave): 1.39 against 1.85 ms at 808 k faces, 24 views of 256 px, P = 8, and 6.41 against 7.38 ms at 4.4 M faces,
//                       48 views of 512 px, P = 5 (profiles/gs_mesh_bake_bench.log, gs_mesh_bake_flat_ab.log).  The thread walks the views in index order with its four sums in registers: no atomics, a
//                       deterministic function of the inputs.
// The camera rows are indexed by the loop counter alone (wave-uniform: scalar loads).  No load is issued before the test that allows it:
// the face indices before the vertices, the pixel range before the depth gather, the depth test before the twelve colour taps.
#include "gs_mesh_common.h"

namespace {

struct BakeGeom {
    int n_views, size, patch, tex, wc;
    float tan_half_fov, z_min, depth_tol, cos_min;
    long n_faces, n_vertices, face_stride;
};

__global__ void bake_clear_kernel(int* __restrict__ status) { *status = 0; }

__global__ __launch_bounds__(256) void gs_mesh_bake_kernel(const float* __restrict__ verts, const float* __restrict__ vert_colours,
                                                           const long* __restrict__ faces, const float* __restrict__ depth,
                                                           const float* __restrict__ colour, const float* __restrict__ views, const BakeGeom g,
                                                           float* __restrict__ out, const size_t plane_stride, int* __restrict__ status) {
    const unsigned P = (unsigned)g.patch, PP = P * P, T = (unsigned)g.tex;
    // blocks are dealt round-robin to the 8 XCDs: give each XCD a contiguous run of cells (gemm_common.h) — neighbouring faces of the mesh,
    // which find each other's vertices and pixels in its L2
    const unsigned blk = (unsigned)vmvg::xcd_logical((int)blockIdx.x, (int)gridDim.x);
    const unsigned idx = blk * 256u + threadIdx.x;                     // T <= 8192: T^2 + 255 < 2^32
    if (idx >= T * T) return;
    const unsigned cell = idx / PP, in_cell = idx - cell * PP;
    const unsigned j = in_cell / P, i = in_cell - j * P;
    const unsigned cx = cell % (unsigned)g.wc, cy = cell / (unsigned)g.wc;
    float* const o = out + (size_t)(cy * P + j) * T + (cx * P + i);
    const bool upper = i + j >= P;
    long vi[3];
    const int unowned = mesh_load_face(faces, g.face_stride, g.n_faces, g.n_vertices, 2L * cell + (upper ? 1 : 0), vi);
    if (unowned > 0) *status = MESH_STATUS_RANGE;                      // every writer stores the same word: a plain store
    if (unowned) {
        o[0] = 0.5f;
        o[plane_stride] = 0.5f;
        o[2 * plane_stride] = 0.5f;
        o[3 * plane_stride] = -1.0f;
        return;
    }
    const float* __restrict__ a = verts + 3 * vi[0];
    const float* __restrict__ b = verts + 3 * vi[1];
    const float* __restrict__ c = verts + 3 * vi[2];
    const float ax = a[0], ay = a[1], az = a[2], bx = b[0], by = b[1], bz = b[2], cx_ = c[0], cy_ = c[1], cz = c[2];
    // barycentrics of the texel centre in the face's own frame: (s - 0.5, t - 0.5) = (i, j), flipped for the upper face; whole numbers
    const float leg = (float)(P - 3);
    float beta = fminf(fmaxf((float)(upper ? P - 1 - i : i) / leg, 0.0f), 1.0f);
    float gamma = fminf(fmaxf((float)(upper ? P - 1 - j : j) / leg, 0.0f), 1.0f);
    const float bg = beta + gamma;
    if (bg > 1.0f) {
        beta = beta / bg;
        gamma = gamma / bg;
    }
    const float alpha = 1.0f - beta - gamma;
    const float wx = alpha * ax + beta * bx + gamma * cx_, wy = alpha * ay + beta * by + gamma * cy_, wz = alpha * az + beta * bz + gamma * cz;
    const float e1x = bx - ax, e1y = by - ay, e1z = bz - az, e2x = cx_ - ax, e2y = cy_ - ay, e2z = cz - az;
    float nx = e1y * e2z - e1z * e2y, ny = e1z * e2x - e1x * e2z, nz = e1x * e2y - e1y * e2x;
    const float len = sqrtf(nx * nx + ny * ny + nz * nz);
    const int n_views = len > 0.0f ? g.n_views : 0;                    // a zero cross product: no view contributes
    nx = nx / len, ny = ny / len, nz = nz / len;                       // (not used when len == 0)
    const float fS = (float)g.size, hi = (float)(g.size - 1);
    const size_t S = (size_t)g.size, SS = S * S;
    float s_r = 0.f, s_g = 0.f, s_b = 0.f, s_w = 0.f;
    for (int v = 0; v < n_views; ++v) {
        const float* __restrict__ m = views + 16 * (size_t)v;          // row-vector convention: [x, 1] @ M
        const auto [xv, yv, z] = mesh_project(m, wx, wy, wz);
        if (!(z > g.z_min)) continue;
        const float inv = 1.0f / (z * g.tan_half_fov);
        const float px = mesh_pixel(xv, inv, fS), py = mesh_pixel(yv, inv, fS);
        if (!(px >= 0.0f && px <= hi && py >= 0.0f && py <= hi)) continue;        // false for NaN: every pixel below lies inside the image
        const float ncx = nx * m[0] + ny * m[4] + nz * m[8], ncy = nx * m[1] + ny * m[5] + nz * m[9], ncz = nx * m[2] + ny * m[6] + nz * m[10];
        const float cosv = -(ncx * xv + ncy * yv + ncz * z) / sqrtf(xv * xv + yv * yv + z * z);
        if (!(cosv > g.cos_min)) continue;
        const float* __restrict__ dmap = depth + (size_t)v * SS;
        const float d = dmap[(size_t)mesh_nearest(py) * S + (size_t)mesh_nearest(px)];   // px + 0.5 <= size - 0.5: the pixel is <= size - 1
        if (d == 0.0f || fabsf(d - z) > g.depth_tol) continue;
        const float fx0 = floorf(px), fy0 = floorf(py);
        const float tx = px - fx0, ty = py - fy0;
        const size_t x0 = (size_t)fx0, y0 = (size_t)fy0;
        const size_t x1 = x0 + 1 < S ? x0 + 1 : S - 1, y1 = y0 + 1 < S ? y0 + 1 : S - 1;
        const float* __restrict__ cm = colour + (size_t)v * 3 * SS;
        const float w = cosv * cosv;
        const float wx0 = 1.0f - tx, wy0 = 1.0f - ty;
        const size_t p00 = y0 * S + x0, p01 = y0 * S + x1, p10 = y1 * S + x0, p11 = y1 * S + x1;
        s_r += w * (wy0 * (wx0 * cm[p00] + tx * cm[p01]) + ty * (wx0 * cm[p10] + tx * cm[p11]));
        s_g += w * (wy0 * (wx0 * cm[SS + p00] + tx * cm[SS + p01]) + ty * (wx0 * cm[SS + p10] + tx * cm[SS + p11]));
        s_b += w * (wy0 * (wx0 * cm[2 * SS + p00] + tx * cm[2 * SS + p01]) + ty * (wx0 * cm[2 * SS + p10] + tx * cm[2 * SS + p11]));
        s_w += w;
    }
    if (s_w > 0.0f) {
        o[0] = s_r / s_w;
        o[plane_stride] = s_g / s_w;
        o[2 * plane_stride] = s_b / s_w;
        o[3 * plane_stride] = s_w;
    } else {                                                           // no view sees the texel: the interpolated vertex colours
        const float* __restrict__ ca = vert_colours + 3 * vi[0];
        const float* __restrict__ cb = vert_colours + 3 * vi[1];
        const float* __restrict__ cc = vert_colours + 3 * vi[2];
        o[0] = alpha * ca[0] + beta * cb[0] + gamma * cc[0];
        o[plane_stride] = alpha * ca[1] + beta * cb[1] + gamma * cc[1];
        o[2 * plane_stride] = alpha * ca[2] + beta * cb[2] + gamma * cc[2];
        o[3 * plane_stride] = 0.0f;
    }
}

}  // namespace

extern "C" int vmv_gs_mesh_bake(const VmvGsMeshBakeParams* pp, void* stream) {
    if (!pp) return VMV_ENULL;
    const VmvGsMeshBakeParams& p = *pp;
    if (!p.verts || !p.vert_colours || !p.faces || !p.depth || !p.colour || !p.views || !p.out || !p.status) return VMV_ENULL;
    const int ef = mesh_check_faces(p.faces, p.face_stride, p.n_faces, 1, p.n_vertices);
    const int ev = mesh_check_views(p.depth, p.colour, p.views, p.n_views, p.size, p.tan_half_fov, p.z_min);
    if (ef == VMV_EINVAL || ev == VMV_EINVAL || p.patch < 4 || !(p.depth_tol > 0.f) || !(p.cos_min >= 0.f && p.cos_min < 1.f)) return VMV_EINVAL;
    // the atlas in 64 bits: Wc = ceil(sqrt(ceil(n_faces / 2))), whatever n_faces is
    const int64_t cells = p.n_faces / 2 + p.n_faces % 2;
    int64_t wc = (int64_t)sqrt((double)cells);
    while (wc * wc < cells) ++wc;
    while (wc > 1 && (wc - 1) * (wc - 1) >= cells) --wc;
    if ((int64_t)p.tex_size != (int64_t)p.patch * wc) return VMV_EINVAL;
    if (p.plane_stride < (int64_t)p.tex_size * p.tex_size) return VMV_EINVAL;
    if (ef == VMV_ERANGE || ev == VMV_ERANGE || p.tex_size > 8192) return VMV_ERANGE;
    if (ef || ev || (((uintptr_t)p.verts | (uintptr_t)p.vert_colours | (uintptr_t)p.out | (uintptr_t)p.status) & 3)) return VMV_EALIGN;
    const hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const BakeGeom g{p.n_views, p.size, p.patch, p.tex_size, (int)wc, p.tan_half_fov, p.z_min, p.depth_tol, p.cos_min,
                     (long)p.n_faces, (long)p.n_vertices, (long)p.face_stride};
    const long n = (long)p.tex_size * p.tex_size;
    hipLaunchKernelGGL(bake_clear_kernel, dim3(1), dim3(1), 0, s, p.status);
    hipLaunchKernelGGL(gs_mesh_bake_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, p.verts, p.vert_colours, (const long*)p.faces,
                       p.depth, p.colour, p.views, g, p.out, (size_t)p.plane_stride, p.status);
    return vmv_launch_status();
}
