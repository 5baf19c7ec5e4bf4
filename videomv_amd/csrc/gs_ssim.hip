// gfx950 (MI355X) — the fit's second objective (videomv_amd/gs_fit.py, loss="l1_dssim"; contract in include/vmv.h, "L1 + D-SSIM"):
//   loss = (1 - lambda) mean|I - T| + lambda (1 - mean SSIM(I, T)),  dL/dI,  and the mean SSIM as a metric.  All fp32.
// SSIM of 3-D Gaussian Splatting / pytorch-ssim: 11-tap Gaussian window (sigma 1.5), zero padding of 5, C1 = 0.01^2, C2 = 0.03^2.
//   gs_ssim_forward_kernel    one block per (plane, 32 x 32 tile): I and T with a 5-pixel halo in LDS, the horizontal pass of the five
//                             window sums (I, T, I^2, T^2, I T) into LDS, the vertical pass into registers (4 rows x 1 column per
//                             thread), then per pixel m and, for the gradient, the three derivative maps (dmu, d11, d12) to the
//                             workspace; per-block partial sums of m and |I - T|
//   gs_ssim_backward_kernel   the same tiling over the three derivative maps (the window is symmetric: the adjoint of the zero-padded
//                             convolution is the same convolution), then dL/dI = (1 - lambda) sign(I - T) / n
//                             - lambda (g*dmu + 2 I g*d11 + T g*d12) / n
//   gs_ssim_final_kernel      the partials summed by one block in a fixed order, in double: deterministic; no atomics anywhere
// Two kernels with the maps in memory rather than one that recomputes them with a 10-pixel halo: the one-launch form measured equal
// or slower inside the fit's iteration and 1.8 x slower as a metric.
#include "common.h"

namespace {

constexpr int SS_TILE = 32;                    // output tile (both directions)
constexpr int SS_R = 5;                        // window radius: 11 taps
constexpr int SS_IN = SS_TILE + 2 * SS_R;      // 42: tile + halo
constexpr int SS_IN_LD = SS_IN + 1;            // 43: odd row stride — the horizontal pass's 4-column strips of 4 rows hit 32 banks
constexpr int SS_H_LD = SS_TILE + 1;           // 33: row stride of the horizontal pass's results (its stores: 4 rows x 8 strips)
constexpr int SS_STRIPS = SS_TILE / 4;         // 4-pixel strips per row (horizontal pass) / per column (vertical pass)
constexpr float SS_C1 = 0.01f * 0.01f, SS_C2 = 0.03f * 0.03f;

// g[i] = exp(-(i - 5)^2 / (2 * 1.5^2)) / sum, normalised in double, rounded to float; g[10 - i] = g[i]
VMV_DEV constexpr float ss_tap(int i) {
    constexpr float g[6] = {0.001028380123898387f, 0.0075987582094967365f, 0.036000773310661316f, 0.10936068743467331f,
                            0.21300554275512695f, 0.26601171493530273f};
    return g[i <= 5 ? i : 10 - i];
}

struct SsimGeom {
    int H, W, tiles_x, tiles_y;
};

// block -> (plane, tile origin)
VMV_DEV void ss_block(const SsimGeom& s, long& plane_off, int& y0, int& x0) {
    const int b = blockIdx.x;
    const int tx = b % s.tiles_x, t = b / s.tiles_x;
    const int ty = t % s.tiles_y, plane = t / s.tiles_y;
    plane_off = (long)plane * s.H * s.W;
    y0 = ty * SS_TILE;
    x0 = tx * SS_TILE;
}

// one plane's tile + halo -> LDS, zeros outside the image (the zero padding of the convolution)
VMV_DEV void ss_stage(float* __restrict__ dst, const float* __restrict__ src, const SsimGeom& s, const int y0, const int x0) {
    for (int i = threadIdx.x; i < SS_IN * SS_IN; i += 256) {
        const int r = i / SS_IN, c = i - r * SS_IN;
        const int y = y0 + r - SS_R, x = x0 + c - SS_R;
        dst[r * SS_IN_LD + c] = (y >= 0 && y < s.H && x >= 0 && x < s.W) ? src[(long)y * s.W + x] : 0.f;
    }
}

// vertical pass: column c, rows r0 .. r0 + 3 of the tile, from the 14 rows r0 .. r0 + 13 of one horizontal result
VMV_DEV void ss_vertical(const float* __restrict__ h, const int r0, const int c, float out[4]) {
#pragma unroll
    for (int j = 0; j < 4; ++j) out[j] = 0.f;
#pragma unroll
    for (int k = 0; k < 14; ++k) {
        const float v = h[(r0 + k) * SS_H_LD + c];
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (k - j >= 0 && k - j <= 10) out[j] += ss_tap(k - j) * v;
    }
}

// dmu / d11 / d12 == nullptr (all three together): scalars only.  The arithmetic of m does not depend on it: same bits either way.
__global__ __launch_bounds__(256) void gs_ssim_forward_kernel(const float* __restrict__ image, const float* __restrict__ target, const SsimGeom s,
                                                              float* __restrict__ dmu, float* __restrict__ d11, float* __restrict__ d12,
                                                              float* __restrict__ part) {
    __shared__ float s_in[2][SS_IN * SS_IN_LD];
    __shared__ float s_h[5][SS_IN * SS_H_LD];
    __shared__ float s_part[2][4];
    long off;
    int y0, x0;
    ss_block(s, off, y0, x0);
    ss_stage(s_in[0], image + off, s, y0, x0);
    ss_stage(s_in[1], target + off, s, y0, x0);
    __syncthreads();
    // horizontal pass: (row of the haloed tile, strip of 4 columns) per thread: 14 + 14 LDS reads for 4 x 5 window sums
    for (int it = threadIdx.x; it < SS_IN * SS_STRIPS; it += 256) {
        const int r = it / SS_STRIPS, c0 = (it - r * SS_STRIPS) * 4;
        float a[14], b[14], aa[14], bb[14], ab[14];
#pragma unroll
        for (int k = 0; k < 14; ++k) {
            a[k] = s_in[0][r * SS_IN_LD + c0 + k];
            b[k] = s_in[1][r * SS_IN_LD + c0 + k];
            aa[k] = a[k] * a[k];
            bb[k] = b[k] * b[k];
            ab[k] = a[k] * b[k];
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float h0 = 0.f, h1 = 0.f, h2 = 0.f, h3 = 0.f, h4 = 0.f;
#pragma unroll
            for (int k = 0; k < 11; ++k) {
                const float w = ss_tap(k);
                h0 += w * a[j + k];
                h1 += w * b[j + k];
                h2 += w * aa[j + k];
                h3 += w * bb[j + k];
                h4 += w * ab[j + k];
            }
            const int o = r * SS_H_LD + c0 + j;
            s_h[0][o] = h0; s_h[1][o] = h1; s_h[2][o] = h2; s_h[3][o] = h3; s_h[4][o] = h4;
        }
    }
    __syncthreads();
    // vertical pass: column c, 4 rows per thread
    const int c = threadIdx.x & 31, r0 = (threadIdx.x >> 5) * 4;
    float mu1[4], mu2[4], e11[4], e22[4], e12[4];
    ss_vertical(s_h[0], r0, c, mu1);
    ss_vertical(s_h[1], r0, c, mu2);
    ss_vertical(s_h[2], r0, c, e11);
    ss_vertical(s_h[3], r0, c, e22);
    ss_vertical(s_h[4], r0, c, e12);
    float sum_m = 0.f, sum_l1 = 0.f;
    const int x = x0 + c;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int y = y0 + r0 + j;
        if (y < s.H && x < s.W) {
            const float m1 = mu1[j], m2 = mu2[j];
            const float s11 = e11[j] - m1 * m1, s22 = e22[j] - m2 * m2, s12 = e12[j] - m1 * m2;
            const float A1 = 2.f * m1 * m2 + SS_C1, A2 = 2.f * s12 + SS_C2;
            const float B1 = m1 * m1 + m2 * m2 + SS_C1, B2 = s11 + s22 + SS_C2;
            const float m = (A1 * A2) / (B1 * B2);
            sum_m += m;
            const int ci = (r0 + j + SS_R) * SS_IN_LD + c + SS_R;
            sum_l1 += fabsf(s_in[0][ci] - s_in[1][ci]);
            if (dmu) {
                const float rB = 1.0f / (B1 * B2);
                const float g11 = -m / B2;                   // dm / d sigma11
                const float g12 = 2.f * A1 * rB;             // dm / d sigma12
                const long o = off + (long)y * s.W + x;
                dmu[o] = 2.f * m2 * A2 * rB - 2.f * m1 * m / B1 - 2.f * m1 * g11 - m2 * g12;
                d11[o] = g11;
                d12[o] = g12;
            }
        }
    }
    const float tm = block_sum(sum_m, s_part[0]);
    const float tl = block_sum(sum_l1, s_part[1]);
    if (threadIdx.x == 0) {
        part[2L * blockIdx.x] = tm;
        part[2L * blockIdx.x + 1] = tl;
    }
}

__global__ __launch_bounds__(256) void gs_ssim_backward_kernel(const float* __restrict__ image, const float* __restrict__ target, const SsimGeom s,
                                                               const float* __restrict__ dmu, const float* __restrict__ d11,
                                                               const float* __restrict__ d12, const float w_l1, const float w_ssim,
                                                               float* __restrict__ dL) {
    __shared__ float s_in[3][SS_IN * SS_IN_LD];
    __shared__ float s_h[3][SS_IN * SS_H_LD];
    long off;
    int y0, x0;
    ss_block(s, off, y0, x0);
    ss_stage(s_in[0], dmu + off, s, y0, x0);
    ss_stage(s_in[1], d11 + off, s, y0, x0);
    ss_stage(s_in[2], d12 + off, s, y0, x0);
    __syncthreads();
    for (int it = threadIdx.x; it < SS_IN * SS_STRIPS; it += 256) {
        const int r = it / SS_STRIPS, c0 = (it - r * SS_STRIPS) * 4;
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            float a[14];
#pragma unroll
            for (int k = 0; k < 14; ++k) a[k] = s_in[q][r * SS_IN_LD + c0 + k];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float h = 0.f;
#pragma unroll
                for (int k = 0; k < 11; ++k) h += ss_tap(k) * a[j + k];
                s_h[q][r * SS_H_LD + c0 + j] = h;
            }
        }
    }
    __syncthreads();
    const int c = threadIdx.x & 31, r0 = (threadIdx.x >> 5) * 4;
    float gmu[4], g11[4], g12[4];
    ss_vertical(s_h[0], r0, c, gmu);
    ss_vertical(s_h[1], r0, c, g11);
    ss_vertical(s_h[2], r0, c, g12);
    const int x = x0 + c;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int y = y0 + r0 + j;
        if (y < s.H && x < s.W) {
            const long o = off + (long)y * s.W + x;
            const float a = image[o], t = target[o];
            const float d = a - t;
            const float sg = d > 0.f ? 1.f : d < 0.f ? -1.f : 0.f;           // sign(0) = 0: ties are common (equal backgrounds)
            dL[o] = w_l1 * sg - w_ssim * (gmu[j] + 2.f * a * g11[j] + t * g12[j]);
        }
    }
}

// loss[0] = (1 - lambda) L1 + lambda (1 - SSIM), loss[1] = L1, loss[2] = mean SSIM
__global__ __launch_bounds__(256) void gs_ssim_final_kernel(const float* __restrict__ part, const int nb, const double inv_n, const float lambda,
                                                            float* __restrict__ loss) {
    __shared__ double s_sum[2][256];
    double m = 0.0, l = 0.0;
    for (int i = threadIdx.x; i < nb; i += 256) {
        m += (double)part[2L * i];
        l += (double)part[2L * i + 1];
    }
    s_sum[0][threadIdx.x] = m;
    s_sum[1][threadIdx.x] = l;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) {
            s_sum[0][threadIdx.x] += s_sum[0][threadIdx.x + o];
            s_sum[1][threadIdx.x] += s_sum[1][threadIdx.x + o];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const double ssim = s_sum[0][0] * inv_n, l1 = s_sum[1][0] * inv_n;
        loss[0] = (float)((1.0 - (double)lambda) * l1 + (double)lambda * (1.0 - ssim));
        loss[1] = (float)l1;
        loss[2] = (float)ssim;
    }
}

// sizes shared by the workspace query and the launcher; VMV_OK or the code both answer
int ssim_sizes(const int planes, const int height, const int width, long& n, long& blocks) {
    if (planes <= 0 || height <= 0 || width <= 0) return VMV_EINVAL;
    n = (long)planes * height * width;
    if (n >= (1L << 31)) return VMV_ERANGE;
    const long tx = (width + SS_TILE - 1) / SS_TILE, ty = (height + SS_TILE - 1) / SS_TILE;
    blocks = tx * ty * planes;
    if (blocks >= (1L << 31)) return VMV_ERANGE;
    return VMV_OK;
}

size_t ssim_workspace(const long n, const long blocks) {
    return ((size_t)(3 * n + 2 * blocks) * sizeof(float) + 255) & ~(size_t)255;
}

}  // namespace

extern "C" int vmv_gs_ssim_loss_workspace_bytes(int planes, int height, int width, size_t* bytes) {
    if (!bytes) return VMV_ENULL;
    long n, blocks;
    const int rc = ssim_sizes(planes, height, width, n, blocks);
    if (rc != VMV_OK) return rc;
    *bytes = ssim_workspace(n, blocks);
    return VMV_OK;
}

extern "C" int vmv_gs_ssim_loss(const VmvGsSsimLossParams* pp, void* stream) {
    if (!pp) return VMV_ENULL;
    const VmvGsSsimLossParams& p = *pp;
    if (!p.image || !p.target || !p.loss || !p.workspace) return VMV_ENULL;
    long n, blocks;
    const int rc = ssim_sizes(p.planes, p.height, p.width, n, blocks);
    if (rc != VMV_OK) return rc;
    if (!(p.lambda_dssim >= 0.f && p.lambda_dssim <= 1.f)) return VMV_EINVAL;
    if (p.workspace_bytes < ssim_workspace(n, blocks)) return VMV_EINVAL;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const SsimGeom s{p.height, p.width, (p.width + SS_TILE - 1) / SS_TILE, (p.height + SS_TILE - 1) / SS_TILE};
    // workspace: the three derivative maps [planes][height][width], then 2 partial sums per block
    float* dmu = p.workspace;
    float* d11 = dmu + n;
    float* d12 = d11 + n;
    float* part = d12 + n;
    const bool grad = p.dL_dimage != nullptr;
    hipLaunchKernelGGL(gs_ssim_forward_kernel, dim3((unsigned)blocks), dim3(256), 0, st, p.image, p.target, s, grad ? dmu : nullptr,
                       grad ? d11 : nullptr, grad ? d12 : nullptr, part);
    if (grad) {
        const float inv_n = (float)(1.0 / (double)n);
        hipLaunchKernelGGL(gs_ssim_backward_kernel, dim3((unsigned)blocks), dim3(256), 0, st, p.image, p.target, s, (const float*)dmu,
                           (const float*)d11, (const float*)d12, (1.0f - p.lambda_dssim) * inv_n, p.lambda_dssim * inv_n, p.dL_dimage);
    }
    hipLaunchKernelGGL(gs_ssim_final_kernel, dim3(1), dim3(256), 0, st, (const float*)part, (int)blocks, 1.0 / (double)n, p.lambda_dssim, p.loss);
    return vmv_launch_status();
}
