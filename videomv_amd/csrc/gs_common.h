// gs_common.h — the one definition of everything the Gaussian rasteriser's forward (raster.hip) and backward (raster_bwd.hip) must agree
// on.  The backward is only correct while it makes the forward's skip / alpha / stop decision for every (pixel, Gaussian) and differentiates
// the forward's own projection, so both include the arithmetic from here instead of restating it.
//
// The blend rule, per pixel and Gaussian in the tile's (depth, index) order:
//   skip   power > 0, and alpha < 1/255 (THE 1/255 CUT: such a Gaussian changes no 8-bit output; a conservative base-2 pre-test on
//          p2 + log2(opacity) against CULL lets a wave skip a pair before the exponential, the exact test follows for what passes);
//   alpha  = min(0.99, opacity e^power) (THE 0.99 CAP keeps 1 - alpha >= 0.01, so the backward can recover T in front of a Gaussian as
//          T / (1 - alpha); where the cap binds, alpha has no gradient to the conic, the centre or the opacity);
//   stop   BEFORE the Gaussian that would take T below 1e-4: that Gaussian is not applied, so the final T stays >= 1e-4 and the backward's
//          divisions start from a normal number.
// THE PAD: the loops take staged Gaussians two at a time, so the entry behind an odd tail is a Gaussian nobody sees — log2(opacity)
// -1e30 fails the pre-test, opacity 0 gives alpha 0 — and its colour is written as 0, not left stale: a pair is blended as a whole when
// either half passes, the failing half with weight 0, and 0 x stale LDS could be 0 x NaN.
#pragma once
#include "common.h"

constexpr int GS_TILE = 16;
constexpr float GS_LOG2E = 1.4426950408889634f;
constexpr float GS_ALPHA_MIN = 1.0f / 255.0f;
constexpr float GS_CULL = -7.9943534f - 0.02f;      // log2(GS_ALPHA_MIN) with a margin
constexpr float SH_C0 = 0.28209479177387814f;

// ---- projection: the forward terms of one Gaussian `g` (14 floats, activated) against one view.  `V` / `M` = cam_view / cam_view_proj
// (row-major, row-vector convention: [m, 1] @ matrix).  gs_project (raster.hip) stores from these, gs_preprocess_backward_kernel
// (raster_bwd.hip) applies the chain rule to these: the forward's bits are the contract, operation order included.
// A statement list, not a function: it declares, in the caller's scope,
//   vx vy vz                 view position                      nx ny iw      NDC and 1 / (w + 1e-7)
//   R[9] s2[3] S3[9]         rotation of the raw quaternion (r, x, y, z) used as given, scale^2, Sigma3 = R diag(s^2) R^T
//   focal lim rx ry tx ty    t.xy = clamp(v.xy / v.z, +-lim) v.z
//   j00 j02 j11 j12          J = [[f/z, 0, -f tx/z^2], [0, f/z, -f ty/z^2]]
//   T0[3] T1[3]              rows of T = J W3, W3[r][c] = V[c*4 + r]             u0[3] u1[3]   Sigma3 T^T
//   ca cb cc                 Sigma2 = T Sigma3 T^T + 0.3 I
// and runs `NEAR_CULL` right behind vz (the forward's first cull: `if (!(vz > 0.2f)) return`).  Every function form tried (terms
// through a struct, by reference, by value, through a continuation) made the compiler vectorise and contract the forward's conic
// differently, which changes its last bits; expanded in place the forward compiles to the instructions it had.
#define GS_PROJECT_TERMS(g, V, M, size, tan_half_fov, NEAR_CULL)                                                                        \
    const float mx = (g)[0], my = (g)[1], mz = (g)[2];                                                                                  \
    const float vx = mx * (V)[0] + my * (V)[4] + mz * (V)[8] + (V)[12];                                                                 \
    const float vy = mx * (V)[1] + my * (V)[5] + mz * (V)[9] + (V)[13];                                                                 \
    const float vz = mx * (V)[2] + my * (V)[6] + mz * (V)[10] + (V)[14];                                                                \
    NEAR_CULL;                                                                                                                          \
    const float hx = mx * (M)[0] + my * (M)[4] + mz * (M)[8] + (M)[12];                                                                 \
    const float hy = mx * (M)[1] + my * (M)[5] + mz * (M)[9] + (M)[13];                                                                 \
    const float hw = mx * (M)[3] + my * (M)[7] + mz * (M)[11] + (M)[15];                                                                \
    const float iw = 1.0f / (hw + 1e-7f);                                                                                               \
    const float nx = hx * iw, ny = hy * iw;                                                                                             \
    const float sx = (g)[4], sy = (g)[5], sz = (g)[6];                                                                                  \
    const float qr = (g)[7], qx = (g)[8], qy = (g)[9], qz = (g)[10];                                                                    \
    const float R[9] = {1.f - 2.f * (qy * qy + qz * qz), 2.f * (qx * qy - qr * qz), 2.f * (qx * qz + qr * qy),                          \
                        2.f * (qx * qy + qr * qz), 1.f - 2.f * (qx * qx + qz * qz), 2.f * (qy * qz - qr * qx),                          \
                        2.f * (qx * qz - qr * qy), 2.f * (qy * qz + qr * qx), 1.f - 2.f * (qx * qx + qy * qy)};                         \
    const float s2[3] = {sx * sx, sy * sy, sz * sz};                                                                                    \
    float S3[9];                                                                                                                        \
    _Pragma("unroll") for (int a = 0; a < 3; ++a)                                                                                       \
        _Pragma("unroll") for (int b = 0; b < 3; ++b)                                                                                   \
            S3[a * 3 + b] = R[a * 3 + 0] * s2[0] * R[b * 3 + 0] + R[a * 3 + 1] * s2[1] * R[b * 3 + 1] + R[a * 3 + 2] * s2[2] * R[b * 3 + 2]; \
    const float focal = (float)(size) / (2.0f * (tan_half_fov));                                                                        \
    const float lim = 1.3f * (tan_half_fov);                                                                                            \
    const float rx = vx / vz, tx = fminf(lim, fmaxf(-lim, rx)) * vz;                                                                    \
    const float ry = vy / vz, ty = fminf(lim, fmaxf(-lim, ry)) * vz;                                                                    \
    const float j00 = focal / vz, j02 = -focal * tx / (vz * vz), j11 = focal / vz, j12 = -focal * ty / (vz * vz);                       \
    float T0[3], T1[3];                                                                                                                 \
    _Pragma("unroll") for (int c = 0; c < 3; ++c) {                                                                                     \
        T0[c] = j00 * (V)[c * 4 + 0] + j02 * (V)[c * 4 + 2];                                                                            \
        T1[c] = j11 * (V)[c * 4 + 1] + j12 * (V)[c * 4 + 2];                                                                            \
    }                                                                                                                                   \
    float u0[3], u1[3];                                                                                                                 \
    _Pragma("unroll") for (int a = 0; a < 3; ++a) {                                                                                     \
        u0[a] = S3[a * 3 + 0] * T0[0] + S3[a * 3 + 1] * T0[1] + S3[a * 3 + 2] * T0[2];                                                  \
        u1[a] = S3[a * 3 + 0] * T1[0] + S3[a * 3 + 1] * T1[1] + S3[a * 3 + 2] * T1[2];                                                  \
    }                                                                                                                                   \
    const float ca = T0[0] * u0[0] + T0[1] * u0[1] + T0[2] * u0[2] + 0.3f;                                                              \
    const float cb = T0[0] * u1[0] + T0[1] * u1[1] + T0[2] * u1[2];                                                                     \
    const float cc = T1[0] * u1[0] + T1[1] * u1[1] + T1[2] * u1[2] + 0.3f

// ---- staged tile: a chunk of up to 256 of a tile's Gaussians in LDS, one array per field (+ 2 pad entries).  The loops take them TWO
// at a time: a field pair is one ds_read_b64 and the pair's falloff exponents are packed fp32 operations (v_pk_*: 8 for two Gaussians
// where the one-at-a-time form issued 16).  The exponent is taken in base 2, so the conic is pre-scaled by -0.5 log2(e) when staged (one
// v_exp_f32 instead of expf's range reduction).  What only one kernel reads — the depth mode's z, the backward's raw conic and Gaussian
// index — is staged by that kernel in arrays of its own, outside this footprint.
struct GsTile {
    float x[258], y[258], A[258], B[258], C[258];      // centre; conic scaled: p2 = A dx^2 + C dy^2 + B dx dy = log2 of the falloff
    float l[258], o[258];                              // log2(opacity) (-1e30 for opacity <= 0), opacity
    float r[258], g[258], b[258];                      // colour
};
// The same fields as ten LDS arrays of the kernel's own (each 258 floats, 16-byte aligned).  The forward blend keeps this form: as ONE LDS
// object the compiler merges the pair loop's reads across fields (three ds_read2_b64 for four reads) and the blend measured 1.1 - 2.2 %
// slower; the backward walk, whose time is in the reductions, measured 0.5 % faster on GsTile and needs 28 B less LDS.
struct GsTileRef { float *x, *y, *A, *B, *C, *l, *o, *r, *g, *b; };
// entry `t` from Gaussian `gi` of the view (`xy` / `co` = the view's preprocess arrays, `gaussians` = its sample's)
template <typename Tile>
VMV_DEV void gs_stage(Tile& s, const int t, const uint32_t gi, const float* __restrict__ xy, const float* __restrict__ co,
                      const float* __restrict__ gaussians) {
    const float* cg = co + 4L * gi;
    const float* g = gaussians + 14L * gi + 11;
    const float o = cg[3];
    s.x[t] = xy[2 * gi]; s.y[t] = xy[2 * gi + 1];
    s.A[t] = -0.5f * GS_LOG2E * cg[0]; s.B[t] = -GS_LOG2E * cg[1]; s.C[t] = -0.5f * GS_LOG2E * cg[2];
    s.l[t] = o > 0.f ? __builtin_amdgcn_logf(o) : -1e30f;      // v_log_f32: log2
    s.o[t] = o;
    s.r[t] = g[0]; s.g[t] = g[1]; s.b[t] = g[2];
}
// entry `t` as the pad (header comment)
template <typename Tile>
VMV_DEV void gs_stage_pad(Tile& s, const int t) {
    s.x[t] = 0.f; s.y[t] = 0.f; s.A[t] = 0.f; s.B[t] = 0.f; s.C[t] = 0.f;
    s.l[t] = -1e30f; s.o[t] = 0.f;
    s.r[t] = 0.f; s.g[t] = 0.f; s.b[t] = 0.f;
}

// ---- pair falloff: the staged pair (k, k + 1), k even, against the lane's pixel (fx, fy) -> p2 = log2 of each falloff there and the
// conservative pre-tests m0 / m1 ("this lane may see it": power <= 0 and p2 + log2(opacity) >= CULL)
struct GsPair { f32x2_t p2; bool m0, m1; };
template <typename Tile>
VMV_DEV GsPair gs_pair_falloff(const Tile& s, const int k, const float fx, const float fy) {
    const f32x2_t fx2 = {fx, fx}, fy2 = {fy, fy};
    const f32x2_t dx = *reinterpret_cast<const f32x2_t*>(s.x + k) - fx2, dy = *reinterpret_cast<const f32x2_t*>(s.y + k) - fy2;
    const f32x2_t p2 = *reinterpret_cast<const f32x2_t*>(s.A + k) * dx * dx + *reinterpret_cast<const f32x2_t*>(s.C + k) * dy * dy +
                       *reinterpret_cast<const f32x2_t*>(s.B + k) * dx * dy;
    const f32x2_t pre = p2 + *reinterpret_cast<const f32x2_t*>(s.l + k);
    return {p2, p2.x <= 0.0f && pre.x >= GS_CULL, p2.y <= 0.0f && pre.y >= GS_CULL};
}
// alpha of staged Gaussian `k` from its falloff G = 2^p2 (the backward also needs G itself); the exact cut is `alpha >= GS_ALPHA_MIN`
VMV_DEV float gs_falloff(const float p2) { return __builtin_amdgcn_exp2f(p2); }
template <typename Tile>
VMV_DEV float gs_alpha(const Tile& s, const int k, const float G) { return fminf(0.99f, s.o[k] * G); }

// ---- tile / view addressing of the batched pass: block (x, y, z) = tile (x, y) of view vv = b * V + v
struct GsTileView {
    int vv;
    long hw, vo, pix;                       // pixels per plane, first (view, Gaussian) record, first pixel of the view's planes
    uint32_t lo, hi;                        // the tile's instances in vals_sorted (0 / 0 from the memset for a tile or view without any)
    const float *xy, *conic_opacity, *gaussians;      // the view's preprocess arrays, its sample's Gaussians
    float *out_color, *out_alpha;           // the view's planes (out_alpha may be null)
};
VMV_DEV GsTileView gs_tile_view(const VmvGsBatchParams& p) {
    const int grid = (p.size + GS_TILE - 1) / GS_TILE;
    GsTileView t;
    t.vv = blockIdx.z;
    const long tile = (long)t.vv * grid * grid + blockIdx.y * grid + blockIdx.x;
    t.hw = (long)p.size * p.size; t.vo = (long)t.vv * p.N; t.pix = t.hw * t.vv;
    t.lo = p.ranges[2 * tile]; t.hi = p.ranges[2 * tile + 1];
    t.xy = p.xy + 2 * t.vo; t.conic_opacity = p.conic_opacity + 4 * t.vo;
    t.gaussians = p.gaussians + (long)(t.vv / p.V) * p.N * 14;
    t.out_color = p.out_color + 3 * t.pix;
    t.out_alpha = p.out_alpha ? p.out_alpha + t.pix : nullptr;
    return t;
}

// ---- range limits every entry point of the batched pass shares: blockIdx.y / .z carry the view, (view, tile) ids are 32-bit keys.
// Each caller adds its own null checks and its own bound on B V N.
inline int gs_batch_limits(const VmvGsBatchParams& p) {
    if (p.B <= 0 || p.V <= 0 || p.N <= 0 || p.size <= 0 || !(p.tan_half_fov > 0.f)) return VMV_EINVAL;
    const long grid = (p.size + GS_TILE - 1) / GS_TILE;
    if ((long)p.B * p.V > 65535 || (long)p.B * p.V * grid * grid >= (1L << 31)) return VMV_ERANGE;
    return VMV_OK;
}
