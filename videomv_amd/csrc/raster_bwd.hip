// raster_bwd.hip — the batched Gaussian-splatting pass of raster.hip, differentiated, plus the image loss and the fused Adam step that
// fit Gaussians to a view set (videomv_amd/gs_fit.py; contract in include/vmv.h, "Fitting Gaussians to a view set").  All fp32.
//
//   gs_blend_backward_kernel    one 256-thread block per (view, 16x16 tile): walks the tile's instances BACK TO FRONT from the largest
//                               n_contrib of its pixels, in the forward's chunks of 256 and with the forward's pair arithmetic (base-2
//                               exponent, pre-scaled conic), recovers T before each Gaussian from the final T, and sums each instance's
//                               9 screen-space gradients over the tile's pixels on chip — a wave reduction, then one LDS add per wave —
//                               before ONE atomicAdd(float*) per value and instance into grad2d (why atomics)
//   gs_preprocess_backward_kernel  one thread per (view, Gaussian): grad2d -> the 14-float activated layout, plain stores
//   gs_view_sum_kernel          grad[b][i] = sum over v of grad_view[b][v][i], in view order (deterministic)
//   gs_loss_partial_kernel / gs_loss_final_kernel   MSE + dL/dimage, per-block partials summed by one block in a fixed order
//   gs_adam_kernel              one thread per Gaussian: activation Jacobians, bias-corrected Adam, activated output
#include "common.h"

namespace {

constexpr int GS_TILE = 16;
constexpr float LOG2E = 1.4426950408889634f;
constexpr float CULL = -7.9943534f - 0.02f;      // raster.hip gs_blend_tile: log2(1 / 255) with a margin
constexpr float SH_C0 = 0.28209479177387814f;

VMV_DEV float wave_sum(float v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

__global__ __launch_bounds__(256) void gs_blend_backward_kernel(const VmvGsBackwardParams q) {
    const VmvGsBatchParams& p = q.pass;
    __shared__ __attribute__((aligned(16))) float s_x[258], s_y[258], s_A[258], s_B[258], s_C[258], s_l[258], s_o[258];
    __shared__ float s_r[256], s_g[256], s_b[256], s_ca[256], s_cb[256], s_cc[256];
    __shared__ uint32_t s_gi[256];
    __shared__ float s_grad[9][256];
    __shared__ int s_max;
    const int grid = (p.size + GS_TILE - 1) / GS_TILE;
    const int vv = blockIdx.z;
    const long tile = (long)vv * grid * grid + blockIdx.y * grid + blockIdx.x;
    const long hw = (long)p.size * p.size, vo = (long)vv * p.N;
    const uint32_t lo = p.ranges[2 * tile];
    const float* xy = p.xy + 2 * vo;
    const float* co = p.conic_opacity + 4 * vo;
    const float* gs = p.gaussians + (long)(vv / p.V) * p.N * 14;
    const int px = blockIdx.x * GS_TILE + (threadIdx.x & 15), py = blockIdx.y * GS_TILE + (threadIdx.x >> 4);
    const bool inside = px < p.size && py < p.size;
    const float fx = (float)px, fy = (float)py;
    int cnt = 0;
    float T = 1.0f, d0 = 0.f, d1 = 0.f, d2 = 0.f;
    if (inside) {
        const long o = (long)py * p.size + px;
        cnt = q.n_contrib[hw * vv + o];
        T = q.final_T[hw * vv + o];
        const float* img = p.out_color + 3 * hw * vv + o;
        const float* dl = q.dL_dimage + 3 * hw * vv + o;
        // clamp(0, 1) of the output: no gradient where it clamped
        d0 = (img[0] > 0.f && img[0] < 1.f) ? dl[0] : 0.f;
        d1 = (img[hw] > 0.f && img[hw] < 1.f) ? dl[hw] : 0.f;
        d2 = (img[2 * hw] > 0.f && img[2 * hw] < 1.f) ? dl[2 * hw] : 0.f;
    }
    if (threadIdx.x == 0) s_max = 0;
#pragma unroll
    for (int f = 0; f < 9; ++f) s_grad[f][threadIdx.x] = 0.f;
    __syncthreads();
    if (cnt > 0) atomicMax(&s_max, cnt);
    __syncthreads();
    const int nmax = s_max;
    const float Tf = T;
    const float bgdot = p.bg[0] * d0 + p.bg[1] * d1 + p.bg[2] * d2;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f;          // colour of what lies behind the current Gaussian, per unit transmittance
    const int lane = threadIdx.x & 63;
    for (int c = (nmax - 1) >> 8; c >= 0 && nmax > 0; --c) {
        const uint32_t base = lo + 256u * (uint32_t)c;
        const int n = min(256, nmax - 256 * c);
        if ((int)threadIdx.x < n) {
            const uint32_t gi = p.vals_sorted[base + threadIdx.x];
            const float* cg = co + 4L * gi;
            const float* g = gs + 14L * gi + 11;
            const float o = cg[3];
            s_x[threadIdx.x] = xy[2 * gi]; s_y[threadIdx.x] = xy[2 * gi + 1];
            s_A[threadIdx.x] = -0.5f * LOG2E * cg[0]; s_B[threadIdx.x] = -LOG2E * cg[1]; s_C[threadIdx.x] = -0.5f * LOG2E * cg[2];
            s_l[threadIdx.x] = o > 0.f ? __builtin_amdgcn_logf(o) : -1e30f;
            s_o[threadIdx.x] = o;
            s_r[threadIdx.x] = g[0]; s_g[threadIdx.x] = g[1]; s_b[threadIdx.x] = g[2];
            s_ca[threadIdx.x] = cg[0]; s_cb[threadIdx.x] = cg[1]; s_cc[threadIdx.x] = cg[2];
            s_gi[threadIdx.x] = gi;
        } else {
            s_x[threadIdx.x] = 0.f; s_y[threadIdx.x] = 0.f; s_A[threadIdx.x] = 0.f; s_B[threadIdx.x] = 0.f; s_C[threadIdx.x] = 0.f;
            s_l[threadIdx.x] = -1e30f; s_o[threadIdx.x] = 0.f;
            s_r[threadIdx.x] = 0.f; s_g[threadIdx.x] = 0.f; s_b[threadIdx.x] = 0.f;
            s_ca[threadIdx.x] = 0.f; s_cb[threadIdx.x] = 0.f; s_cc[threadIdx.x] = 0.f; s_gi[threadIdx.x] = 0u;
        }
        __syncthreads();
        auto back_one = [&](const int k, const float p2, const bool maybe) {
            const int jr = 256 * c + k;
            const float G = __builtin_amdgcn_exp2f(p2);
            const float ag = s_o[k] * G;
            const float alpha = fminf(0.99f, ag);
            const bool hit = maybe && jr < cnt && alpha >= 1.0f / 255.0f;
            if (__builtin_amdgcn_ballot_w64(hit) == 0) return;
            float g[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            if (hit) {
                const float om = 1.0f - alpha;
                T = T / om;                      // transmittance in front of this Gaussian
                const float w = alpha * T;
                g[6] = w * d0; g[7] = w * d1; g[8] = w * d2;
                const float dla = T * ((s_r[k] - a0) * d0 + (s_g[k] - a1) * d1 + (s_b[k] - a2) * d2) - Tf / om * bgdot;
                a0 = alpha * s_r[k] + om * a0; a1 = alpha * s_g[k] + om * a1; a2 = alpha * s_b[k] + om * a2;
                if (ag < 0.99f) {                // alpha = o e^power below the cap
                    const float dlp = dla * alpha;
                    const float dx = s_x[k] - fx, dy = s_y[k] - fy;
                    g[0] = -dlp * (s_ca[k] * dx + s_cb[k] * dy);
                    g[1] = -dlp * (s_cc[k] * dy + s_cb[k] * dx);
                    g[2] = -0.5f * dlp * dx * dx;
                    g[3] = -dlp * dx * dy;
                    g[4] = -0.5f * dlp * dy * dy;
                    g[5] = dla * G;
                }
            }
#pragma unroll
            for (int f = 0; f < 9; ++f) {
                const float s = wave_sum(g[f]);
                if (lane == 0 && s != 0.f) atomicAdd(&s_grad[f][k], s);
            }
        };
        const f32x2_t fx2 = {fx, fx}, fy2 = {fy, fy};
        for (int k = (n - 1) & ~1; k >= 0; k -= 2) {      // the forward's pairs (k, k + 1), k even, taken in reverse
            const f32x2_t dx = *reinterpret_cast<const f32x2_t*>(s_x + k) - fx2, dy = *reinterpret_cast<const f32x2_t*>(s_y + k) - fy2;
            const f32x2_t p2 = *reinterpret_cast<const f32x2_t*>(s_A + k) * dx * dx + *reinterpret_cast<const f32x2_t*>(s_C + k) * dy * dy +
                               *reinterpret_cast<const f32x2_t*>(s_B + k) * dx * dy;
            const f32x2_t pre = p2 + *reinterpret_cast<const f32x2_t*>(s_l + k);
            const bool m0 = p2.x <= 0.0f && pre.x >= CULL, m1 = p2.y <= 0.0f && pre.y >= CULL;
            if (__builtin_amdgcn_ballot_w64((m0 && k < cnt - 256 * c) || (m1 && k + 1 < cnt - 256 * c)) == 0) continue;
            back_one(k + 1, p2.y, m1);
            back_one(k, p2.x, m0);
        }
        __syncthreads();
        for (int idx = threadIdx.x; idx < 9 * n; idx += 256) {
            const int slot = idx / 9, f = idx - 9 * slot;
            const float v = s_grad[f][slot];
            if (v != 0.f) atomicAdd(q.grad2d + (vo + s_gi[slot]) * 9 + f, v);
            s_grad[f][slot] = 0.f;
        }
        __syncthreads();
    }
}

// One (view, Gaussian): the screen-space gradients back through gs_project (raster.hip) to the activated 14-float layout.
__global__ __launch_bounds__(256) void gs_preprocess_backward_kernel(const VmvGsBackwardParams q) {
    const VmvGsBatchParams& p = q.pass;
    __shared__ float s_m[32];
    const int vv = blockIdx.y;
    if (threadIdx.x < 16) s_m[threadIdx.x] = p.views[16 * vv + threadIdx.x];
    else if (threadIdx.x < 32) s_m[threadIdx.x] = p.view_projs[16 * vv + threadIdx.x - 16];
    __syncthreads();
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= p.N) return;
    const long o = (long)vv * p.N + i;
    float* out = q.grad_view + 14 * o;
    if (p.tiles_touched[o] == 0) {               // culled or off screen: no gradient
#pragma unroll
        for (int f = 0; f < 14; ++f) out[f] = 0.f;
        return;
    }
    const float* V = s_m;
    const float* M = s_m + 16;
    const float* g = p.gaussians + ((long)(vv / p.V) * p.N + i) * 14;
    const float* g2 = q.grad2d + 9 * o;
    const float mx = g[0], my = g[1], mz = g[2];
    const float vx = mx * V[0] + my * V[4] + mz * V[8] + V[12];
    const float vy = mx * V[1] + my * V[5] + mz * V[9] + V[13];
    const float vz = mx * V[2] + my * V[6] + mz * V[10] + V[14];
    const float hx = mx * M[0] + my * M[4] + mz * M[8] + M[12];
    const float hy = mx * M[1] + my * M[5] + mz * M[9] + M[13];
    const float hw = mx * M[3] + my * M[7] + mz * M[11] + M[15];
    const float iw = 1.0f / (hw + 1e-7f);
    const float nx = hx * iw, ny = hy * iw;
    const float sx = g[4], sy = g[5], sz = g[6];
    const float qr = g[7], qx = g[8], qy = g[9], qz = g[10];
    const float R[9] = {1.f - 2.f * (qy * qy + qz * qz), 2.f * (qx * qy - qr * qz), 2.f * (qx * qz + qr * qy),
                        2.f * (qx * qy + qr * qz), 1.f - 2.f * (qx * qx + qz * qz), 2.f * (qy * qz - qr * qx),
                        2.f * (qx * qz - qr * qy), 2.f * (qy * qz + qr * qx), 1.f - 2.f * (qx * qx + qy * qy)};
    const float s2[3] = {sx * sx, sy * sy, sz * sz};
    float S3[9];
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b)
            S3[a * 3 + b] = R[a * 3 + 0] * s2[0] * R[b * 3 + 0] + R[a * 3 + 1] * s2[1] * R[b * 3 + 1] + R[a * 3 + 2] * s2[2] * R[b * 3 + 2];
    const float focal = (float)p.size / (2.0f * p.tan_half_fov);
    const float lim = 1.3f * p.tan_half_fov;
    const float rx = vx / vz, ry = vy / vz;
    const float tx = fminf(lim, fmaxf(-lim, rx)) * vz;
    const float ty = fminf(lim, fmaxf(-lim, ry)) * vz;
    const float iz = 1.0f / vz;
    const float j00 = focal * iz, j02 = -focal * tx * iz * iz, j12 = -focal * ty * iz * iz;
    float T0[3], T1[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        T0[c] = j00 * V[c * 4 + 0] + j02 * V[c * 4 + 2];
        T1[c] = j00 * V[c * 4 + 1] + j12 * V[c * 4 + 2];
    }
    float u0[3], u1[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        u0[a] = S3[a * 3 + 0] * T0[0] + S3[a * 3 + 1] * T0[1] + S3[a * 3 + 2] * T0[2];
        u1[a] = S3[a * 3 + 0] * T1[0] + S3[a * 3 + 1] * T1[1] + S3[a * 3 + 2] * T1[2];
    }
    const float ca = T0[0] * u0[0] + T0[1] * u0[1] + T0[2] * u0[2] + 0.3f;
    const float cb = T0[0] * u1[0] + T0[1] * u1[1] + T0[2] * u1[2];
    const float cc = T1[0] * u1[0] + T1[1] * u1[1] + T1[2] * u1[2] + 0.3f;
    const float idet = 1.0f / (ca * cc - cb * cb);
    const float id2 = idet * idet;
    // conic (A, B, C) = (cc, -cb, ca) / det
    const float gA = g2[2], gB = g2[3], gC = g2[4];
    const float dca = -gA * cc * cc * id2 + gB * cb * cc * id2 + gC * (idet - ca * cc * id2);
    const float dcc = gA * (idet - cc * ca * id2) + gB * cb * ca * id2 - gC * ca * ca * id2;
    const float dcb = 2.f * gA * cc * cb * id2 - gB * (idet + 2.f * cb * cb * id2) + 2.f * gC * ca * cb * id2;
    // Sigma2 = T Sigma3 T^T (+0.3 I)
    float dT0[3], dT1[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        dT0[a] = 2.f * dca * u0[a] + dcb * u1[a];
        dT1[a] = dcb * u0[a] + 2.f * dcc * u1[a];
    }
    float dS[9];
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b) dS[a * 3 + b] = dca * T0[a] * T0[b] + dcb * T0[a] * T1[b] + dcc * T1[a] * T1[b];
    // Sigma3 = R diag(s^2) R^T
    float dR[9], ds[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        float acc = 0.f;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            float t = 0.f;
#pragma unroll
            for (int b = 0; b < 3; ++b) {
                t += (dS[a * 3 + b] + dS[b * 3 + a]) * R[b * 3 + k];
                acc += dS[a * 3 + b] * R[a * 3 + k] * R[b * 3 + k];
            }
            dR[a * 3 + k] = s2[k] * t;
        }
        ds[k] = 2.f * g[4 + k] * acc;
    }
    // T = J W3, W3[r][c] = V[c * 4 + r]; J = [[f/z, 0, -f tx/z^2], [0, f/z, -f ty/z^2]]
    float dj00 = 0.f, dj02 = 0.f, dj11 = 0.f, dj12 = 0.f;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        dj00 += dT0[c] * V[c * 4 + 0]; dj02 += dT0[c] * V[c * 4 + 2];
        dj11 += dT1[c] * V[c * 4 + 1]; dj12 += dT1[c] * V[c * 4 + 2];
    }
    float dvz = -focal * iz * iz * (dj00 + dj11) + 2.f * focal * iz * iz * iz * (tx * dj02 + ty * dj12);
    const float dtx = -focal * iz * iz * dj02, dty = -focal * iz * iz * dj12;
    float dvx = 0.f, dvy = 0.f;
    // t.xy = clamp(t.xy / t.z, +-lim) t.z: unclamped -> t.xy itself; clamped -> +-lim t.z
    if (rx > -lim && rx < lim) dvx += dtx; else dvz += dtx * (rx > 0.f ? lim : -lim);
    if (ry > -lim && ry < lim) dvy += dty; else dvz += dty * (ry > 0.f ? lim : -lim);
    // screen centre ((ndc + 1) size - 1) / 2 of the projective divide
    const float dnx = 0.5f * (float)p.size * g2[0], dny = 0.5f * (float)p.size * g2[1];
    const float dhx = dnx * iw, dhy = dny * iw, dhw = -(dnx * nx + dny * ny) * iw;
#pragma unroll
    for (int a = 0; a < 3; ++a)
        out[a] = dvx * V[a * 4 + 0] + dvy * V[a * 4 + 1] + dvz * V[a * 4 + 2] + dhx * M[a * 4 + 0] + dhy * M[a * 4 + 1] + dhw * M[a * 4 + 3];
    out[3] = g2[5];
    out[4] = ds[0]; out[5] = ds[1]; out[6] = ds[2];
    // R from the raw quaternion (r, x, y, z)
    out[7] = 2.f * (-qz * dR[1] + qy * dR[2] + qz * dR[3] - qx * dR[5] - qy * dR[6] + qx * dR[7]);
    out[8] = 2.f * (qy * dR[1] + qz * dR[2] + qy * dR[3] - 2.f * qx * dR[4] - qr * dR[5] + qz * dR[6] + qr * dR[7] - 2.f * qx * dR[8]);
    out[9] = 2.f * (-2.f * qy * dR[0] + qx * dR[1] + qr * dR[2] + qx * dR[3] + qz * dR[5] - qr * dR[6] + qz * dR[7] - 2.f * qy * dR[8]);
    out[10] = 2.f * (-2.f * qz * dR[0] - qr * dR[1] + qx * dR[2] + qr * dR[3] - 2.f * qz * dR[4] + qy * dR[5] + qx * dR[6] + qy * dR[7]);
    out[11] = g2[6]; out[12] = g2[7]; out[13] = g2[8];
}

__global__ __launch_bounds__(256) void gs_view_sum_kernel(const float* __restrict__ grad_view, float* __restrict__ grad, const int B,
                                                          const int V, const int N) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;          // element of [B][N][14]
    const long per = (long)N * 14;
    if (e >= (long)B * per) return;
    const long b = e / per, r = e - b * per;
    const float* src = grad_view + b * V * per + r;
    float s = 0.f;
    for (int v = 0; v < V; ++v) s += src[v * per];
    grad[e] = s;
}

constexpr int LOSS_BLOCKS = 1024;

VMV_DEV float block_sum(float v, float* s_part) {
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = v;
    __syncthreads();
    return s_part[0] + s_part[1] + s_part[2] + s_part[3];
}

__global__ __launch_bounds__(256) void gs_loss_partial_kernel(const float* __restrict__ image, const float* __restrict__ target, const long n,
                                                              float* __restrict__ dL, float* __restrict__ part) {
    __shared__ float s_part[4];
    const float scale = 2.0f / (float)n;
    float s = 0.f;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
        const float d = image[i] - target[i];
        s += d * d;
        if (dL) dL[i] = scale * d;
    }
    const float t = block_sum(s, s_part);
    if (threadIdx.x == 0) part[blockIdx.x] = t;
}

__global__ __launch_bounds__(256) void gs_loss_final_kernel(const float* __restrict__ part, const int nb, const long n, float* __restrict__ loss) {
    __shared__ float s_part[4];
    float s = 0.f;
    for (int i = threadIdx.x; i < nb; i += 256) s += part[i];
    const float t = block_sum(s, s_part);
    if (threadIdx.x == 0) loss[0] = t / (float)n;
}

__global__ __launch_bounds__(256) void gs_adam_kernel(const VmvGsAdamParams p, const float bc1, const float bc2_sqrt) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= p.n) return;
    float* x = p.params + 14L * i;
    float* out = p.gaussians + 14L * i;
    float w[14];
#pragma unroll
    for (int f = 0; f < 14; ++f) w[f] = x[f];
    if (p.step > 0) {
        const float* gr = p.grad + 14L * i;
        float g[14];
#pragma unroll
        for (int f = 0; f < 14; ++f) g[f] = gr[f];
        // activation Jacobians: raw-parameter gradient from the activated-layout one
        const float sg = 1.0f / (1.0f + expf(-w[3]));
        g[3] *= sg * (1.0f - sg);
#pragma unroll
        for (int f = 4; f < 7; ++f) g[f] *= expf(w[f]);
        const float qn2 = w[7] * w[7] + w[8] * w[8] + w[9] * w[9] + w[10] * w[10];
        const float iq = 1.0f / fmaxf(sqrtf(qn2), 1e-12f);
        const float dot = (w[7] * g[7] + w[8] * g[8] + w[9] * g[9] + w[10] * g[10]) * iq * iq;
#pragma unroll
        for (int f = 7; f < 11; ++f) g[f] = (g[f] - w[f] * dot) * iq;
#pragma unroll
        for (int f = 11; f < 14; ++f) g[f] *= SH_C0;
        float* m = p.m + 14L * i;
        float* v = p.v + 14L * i;
#pragma unroll
        for (int f = 0; f < 14; ++f) {
            const int grp = f < 3 ? 0 : f < 4 ? 1 : f < 7 ? 2 : f < 11 ? 3 : 4;
            const float mf = p.beta1 * m[f] + (1.0f - p.beta1) * g[f];
            const float vf = p.beta2 * v[f] + (1.0f - p.beta2) * g[f] * g[f];
            m[f] = mf; v[f] = vf;
            w[f] -= (p.lr[grp] / bc1) * mf / (sqrtf(vf) / bc2_sqrt + p.eps);
            x[f] = w[f];
        }
    }
#pragma unroll
    for (int f = 0; f < 3; ++f) out[f] = w[f];
    out[3] = 1.0f / (1.0f + expf(-w[3]));
#pragma unroll
    for (int f = 4; f < 7; ++f) out[f] = expf(w[f]);
    const float iq = 1.0f / fmaxf(sqrtf(w[7] * w[7] + w[8] * w[8] + w[9] * w[9] + w[10] * w[10]), 1e-12f);
#pragma unroll
    for (int f = 7; f < 11; ++f) out[f] = w[f] * iq;
#pragma unroll
    for (int f = 11; f < 14; ++f) out[f] = SH_C0 * w[f] + 0.5f;
}

int gs_bwd_check(const VmvGsBackwardParams& q) {
    const VmvGsBatchParams& p = q.pass;
    if (!p.gaussians || !p.views || !p.view_projs || !p.xy || !p.conic_opacity || !p.tiles_touched || !p.ranges || !p.out_color ||
        !q.final_T || !q.n_contrib || !q.dL_dimage || !q.grad2d || !q.grad_view || !q.grad)
        return VMV_ENULL;
    if (p.B <= 0 || p.V <= 0 || p.N <= 0 || p.size <= 0 || !(p.tan_half_fov > 0.f) || p.num_rendered < 0) return VMV_EINVAL;
    const long grid = (p.size + GS_TILE - 1) / GS_TILE;
    if ((long)p.B * p.V > 65535 || (long)p.B * p.V * p.N * 14 >= (1L << 31) || (long)p.B * p.V * grid * grid >= (1L << 31)) return VMV_ERANGE;
    if (p.num_rendered > 0 && !p.vals_sorted) return VMV_ENULL;
    return VMV_OK;
}

}  // namespace

extern "C" int vmv_gs_batch_backward(const VmvGsBackwardParams* qp, void* stream) {
    if (!qp) return VMV_ENULL;
    const VmvGsBackwardParams& q = *qp;
    const int rc = gs_bwd_check(q);
    if (rc != VMV_OK) return rc;
    const VmvGsBatchParams& p = q.pass;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int grid = (p.size + GS_TILE - 1) / GS_TILE;
    const int VV = p.B * p.V;
    const long vn = (long)VV * p.N;
    hipError_t e = hipMemsetAsync(q.grad2d, 0, sizeof(float) * 9 * vn, st);
    if (e != hipSuccess) return (int)e;
    if (p.num_rendered > 0) hipLaunchKernelGGL(gs_blend_backward_kernel, dim3(grid, grid, VV), dim3(256), 0, st, q);
    hipLaunchKernelGGL(gs_preprocess_backward_kernel, dim3((p.N + 255) / 256, VV), dim3(256), 0, st, q);
    const long nout = (long)p.B * p.N * 14;
    hipLaunchKernelGGL(gs_view_sum_kernel, dim3((unsigned)((nout + 255) / 256)), dim3(256), 0, st, (const float*)q.grad_view, q.grad, p.B, p.V, p.N);
    return vmv_launch_status();
}

extern "C" int vmv_gs_image_loss(const float* image, const float* target, long n, float* dL_dimage, float* loss, float* workspace, void* stream) {
    if (!image || !target || !loss || !workspace) return VMV_ENULL;
    if (n <= 0) return VMV_EINVAL;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const long want = (n + 255) / 256;
    const int nb = (int)(want < LOSS_BLOCKS ? want : LOSS_BLOCKS);
    hipLaunchKernelGGL(gs_loss_partial_kernel, dim3(nb), dim3(256), 0, st, image, target, n, dL_dimage, workspace);
    hipLaunchKernelGGL(gs_loss_final_kernel, dim3(1), dim3(256), 0, st, (const float*)workspace, nb, n, loss);
    return vmv_launch_status();
}

extern "C" int vmv_gs_adam_step(const VmvGsAdamParams* pp, void* stream) {
    if (!pp) return VMV_ENULL;
    const VmvGsAdamParams& p = *pp;
    if (!p.params || !p.gaussians) return VMV_ENULL;
    if (p.step > 0 && (!p.m || !p.v || !p.grad)) return VMV_ENULL;
    if (p.n <= 0 || p.step < 0 || (long)p.n * 14 >= (1L << 31)) return VMV_EINVAL;
    const float bc1 = p.step > 0 ? 1.0f - (float)pow((double)p.beta1, (double)p.step) : 1.0f;
    const float bc2 = p.step > 0 ? 1.0f - (float)pow((double)p.beta2, (double)p.step) : 1.0f;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(gs_adam_kernel, dim3((p.n + 255) / 256), dim3(256), 0, st, p, bc1, sqrtf(bc2));
    return vmv_launch_status();
}
