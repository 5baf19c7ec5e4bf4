// gfx950 (MI355X) — what gs_tsdf.hip, gs_mesh_cc.hip and gs_mesh_bake.hip share: where a world point lands in a view (baking tests a
// surface point against the depth map that fusion read), how a face is read, the status bits, what is refused of a faces or views operand.
#pragma once
#include "gemm_common.h"                                               // vmvg::xcd_logical alone
#pragma clang fp contract(off)                                         // file scope, so the including kernels too: a kernel's own pragma would not reach an inlined callee
constexpr int MESH_STATUS_RANGE = 1, MESH_STATUS_GAVE_UP = 2;          // videomv_amd/_lib.py names the same two
constexpr int MESH_MAX_VIEW_SIZE = 32768;                              // the kernels' 32-bit pixel offsets
struct MeshViewPoint { float xv, yv, z; };
// [x, 1] @ M, row-vector convention.  Explicit fused multiply-adds: the same instructions wherever the call stands (every position of
// the TSDF batch, either kernel), so a view gives the same bits wherever a call's split puts it
VMV_DEV MeshViewPoint mesh_project(const float* __restrict__ m, const float wx, const float wy, const float wz) {
    return {fmaf(wz, m[8], fmaf(wy, m[4], fmaf(wx, m[0], m[12]))), fmaf(wz, m[9], fmaf(wy, m[5], fmaf(wx, m[1], m[13]))),
            fmaf(wz, m[10], fmaf(wy, m[6], fmaf(wx, m[2], m[14])))};
}
// the continuous pixel coordinate ((x inv + 1) S - 1) / 2 of view coordinate x, inv = 1 / (z tan_half_fov): one reciprocal serves x and y
VMV_DEV float mesh_pixel(const float x, const float inv, const float fS) { return fmaf(fmaf(x, inv, 1.0f), fS, -1.0f) * 0.5f; }
VMV_DEV float mesh_nearest(const float px) { return floorf(px + 0.5f); }          // the pixel whose centre is nearest
VMV_DEV bool mesh_in_range(long v, long n) { return (unsigned long)v < (unsigned long)n; }
// the vertices of face f -> i.  0: all inside [0, n_vertices); MESH_STATUS_RANGE: one lies outside (i must not be used); -1: f is no face
VMV_DEV int mesh_load_face(const long* __restrict__ faces, long face_stride, long n_faces, long n_vertices, long f, long (&i)[3]) {
    if (f >= n_faces) return -1;
    const long* __restrict__ t = faces + f * face_stride;
    i[0] = t[0], i[1] = t[1], i[2] = t[2];
    return mesh_in_range(i[0], n_vertices) && mesh_in_range(i[1], n_vertices) && mesh_in_range(i[2], n_vertices) ? 0 : MESH_STATUS_RANGE;
}
// Host: the first refusal of an operand in the order invalid, range, alignment (VMV_OK: none); an entry point with more to check asks class by class
inline int mesh_check_faces(const void* faces, int64_t face_stride, int64_t n_faces, int64_t min_faces, int64_t n_vertices) {
    if (n_vertices < 1 || n_faces < min_faces || face_stride < 3) return VMV_EINVAL;
    if (n_vertices > 0x7fffffffL || n_faces > 0x7fffffffL) return VMV_ERANGE;          // int32 labels; one thread per face
    return ((uintptr_t)faces & 7) ? VMV_EALIGN : VMV_OK;
}
inline int mesh_check_views(const void* depth, const void* colour, const void* views, int n_views, int size, float tan_half_fov, float z_min) {
    if (n_views < 1 || size < 1 || !(tan_half_fov > 0.f) || !(z_min > 0.f)) return VMV_EINVAL;
    if (size > MESH_MAX_VIEW_SIZE) return VMV_ERANGE;
    return (((uintptr_t)depth | (uintptr_t)colour | (uintptr_t)views) & 3) ? VMV_EALIGN : VMV_OK;
}
