// gemm_common.h — pieces shared by every GEMM kernel (gemm.hip and the gemm_*.hip / conv_halo.hip family): the XCD-aware block -> tile
// map and its grouped order, the host check that an operand is addressable with 32-bit byte offsets, the K-segment row gather of the
// register-staged kernel and the fused epilogue.
#pragma once
#include "common.h"

namespace vmvg {

constexpr int BK = 64;
// LayerNorm folded into the GEMM with the row statistics taken in its own main loop (vmv.h: VmvGemmParams.ln_eps)
inline bool vmv_gemm_ln_inline(const VmvGemmParams& p) { return !p.rowstat && p.colsum && p.ln_eps > 0.f; }
constexpr int VMV_GLDS_UNSUPPORTED = -100;   // internal: the LDS-DMA kernel cannot address these operands

// ---- XCD-aware block -> tile map.  Blocks are dealt round-robin to the 8 XCDs (block b runs on XCD b & 7); the map gives XCD x the
//      x-th CONTIGUOUS share of the logical ids — the first nblk & 7 shares one longer — so that the blocks an XCD runs at the same
//      time are neighbours and share operands in its L2.  Bijective on [0, nblk) for every nblk (tests/test_abi_cpu.py).
__host__ __device__ __forceinline__ int xcd_logical(const int bid, const int nblk) {
    const int q = nblk >> 3, r = nblk & 7;
    const int xcd = bid & 7, idx = bid >> 3;
    return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
}
// Block -> (row tile, column tile).  gm = 1: the N tiles of one row tile are adjacent — the 32 CUs of an XCD then share A and pull 32
// different W slices in from the fabric once PER ROW TILE (profiles/r6_gemm_traffic_by_kernel.tsv: the 7680 x 10240 x 1280 GEGLU
// fetched 834 MB for 46 MB of operands = W x 30 row tiles).  Grouped order (gm > 1, round 6): consecutive logical ids walk gm row
// tiles, then the next N tile, so the blocks an XCD runs together cover gm row tiles x conc / gm column tiles: a W slice is fetched
// once per gm row tiles and an A slice once per conc / gm column tiles.  The last group is clipped to the row tiles that are left.
__host__ __device__ __forceinline__ void tile_of_block(const int bid, const int tiles_m, const int tiles_n, const int gm, int& tile_m, int& tile_n) {
    const int logical = xcd_logical(bid, tiles_m * tiles_n);
    if (gm > 1) {
        const int gsz = gm * tiles_n, g = logical / gsz, first = g * gm;
        const int gmh = tiles_m - first < gm ? tiles_m - first : gm;
        const int rem = logical - g * gsz;
        tile_n = rem / gmh; tile_m = first + (rem - tile_n * gmh);
    } else {
        tile_m = logical / tiles_n; tile_n = logical - tile_m * tiles_n;
    }
}
// rows of the tile group (gm above): minimises the bytes the `conc` blocks an XCD runs at once (32 CUs x blocks per CU) pull in per K
// chunk, gm x BM + conc / gm x BN, with conc / gm <= the N tiles there are; 1 = the ungrouped order.
// (C symbol for tests and tools: vmv_gemm_group_m, gemm.hip)
inline int gemm_group_m(int tiles_m, int tiles_n, int BM, int BN, int conc) {
    if (tiles_n < 2 || tiles_m < 2) return 1;
    int best = 1, best_cost = BM + conc * BN;
    for (int gm = 2; gm <= conc; gm *= 2) {
        const int gn = (conc + gm - 1) / gm;
        if (gn > tiles_n || gm > tiles_m) continue;
        const int cost = gm * BM + gn * BN;
        if (cost < best_cost) { best = gm; best_cost = cost; }
    }
    return best;
}

// ---- host: 32-bit byte offsets (buffer descriptors, packed lane offsets) reach an operand of `rows` rows of `ld` elements only if it
//      spans < 2 GiB; 64 KB are left for the offsets a kernel adds beyond its last row.
inline bool vmv_span32(long rows, long ld, int elem_bytes = 2) { return rows * ld * elem_bytes < (1L << 31) - 65536; }
// rows of the largest source tensor a gather of *p may touch (a convolution's input can have more rows than its output)
inline long vmv_gemm_src_rows(const VmvGemmParams& p) {
    long maxrows = p.M;
    if (p.OH > 0) { const long src_rows = (long)(p.M / (p.OH * p.OW) + 1) * p.IH * p.IW; if (src_rows > maxrows) maxrows = src_rows; }
    return maxrows;
}
// every operand of *p a kernel addresses with 32-bit byte offsets: every segment's source over a_rows rows, W over N + w_pad_rows rows
// (tiles that read past N), and — where the kernel addresses them that way: rows > 0 — the output and the residual
inline bool vmv_gemm_spans32(const VmvGemmParams& p, long a_rows, int w_pad_rows, long out_rows, long res_rows) {
    for (int i = 0; i < p.nseg; ++i)
        if (!vmv_span32(a_rows, p.seg[i].ld)) return false;
    if (!vmv_span32((long)p.N + w_pad_rows, p.ktot)) return false;
    if (out_rows > 0 && !vmv_span32(out_rows, p.ldo, p.out_fp32 ? 4 : 2)) return false;
    if (res_rows > 0 && p.residual && !vmv_span32(res_rows, p.ldr)) return false;
    return true;
}

struct RowInfo {
    int m;       // global row (or -1 when out of range)
    int nb;      // spatial: image base row (n * IH * IW)
    int oy, ox;  // spatial: output pixel
    int fr;      // temporal: frame index
};

VMV_DEV int seg_row_offset(const VmvGemmParams& p, const VmvGemmSeg& sg, const RowInfo& r) {
    // element offset of the source row feeding output row r for this segment, or -1 (zero row)
    if (r.m < 0) return -1;
    if (sg.mode == VMV_SEG_LINEAR) return r.m * sg.ld;
    if (sg.mode == VMV_SEG_SPATIAL) {
        const int iy = r.oy * p.stride + sg.d0;
        const int ix = r.ox * p.stride + sg.d1;
        const int VH = p.IH << p.ups, VW = p.IW << p.ups;
        if (iy < 0 || iy >= VH || ix < 0 || ix >= VW) return -1;
        return (r.nb + (iy >> p.ups) * p.IW + (ix >> p.ups)) * sg.ld;
    }
    // temporal
    const int f = r.fr + sg.d0;
    if (f < 0 || f >= p.F) return -1;
    return (r.m + sg.d0 * p.P) * sg.ld;
}

// Epilogue for 4 consecutive output channels [n, n+4) of row m.  v = accumulators (x half for GEGLU),
// g = gate accumulators (GEGLU only).  `n` indexes W rows (pre-GEGLU numbering).
VMV_DEV void epilogue_store(const VmvGemmParams& p, int m, int n, f32x4_t v, f32x4_t g) {
    if (m >= p.M || n >= p.N) return;
    if (p.rowstat) {       // LayerNorm folded into this GEMM (vmv.h): rstd * (acc - mean * colsum[n])
        const float2 ms = *reinterpret_cast<const float2*>(p.rowstat + (size_t)m * 2);
        const f32x4_t c0 = *reinterpret_cast<const f32x4_t*>(p.colsum + n);
        v = (v - c0 * ms.x) * ms.y;
        if (p.epilogue == VMV_EPI_GEGLU) {
            const f32x4_t c1 = *reinterpret_cast<const f32x4_t*>(p.colsum + n + 16);
            g = (g - c1 * ms.x) * ms.y;
        }
    }
    if (p.bias) {
        const f32x4_t b = *reinterpret_cast<const f32x4_t*>(p.bias + n);
        v += b;
        if (p.epilogue == VMV_EPI_GEGLU) g += *reinterpret_cast<const f32x4_t*>(p.bias + n + 16);
    }
    int no = n;
    if (p.epilogue == VMV_EPI_GEGLU) {
        v.x *= gelu_erf_f(g.x); v.y *= gelu_erf_f(g.y); v.z *= gelu_erf_f(g.z); v.w *= gelu_erf_f(g.w);
        no = (n >> 5) * 16 + (n & 15);
    }
    if (p.rowvec) {
        const f32x4_t rv = *reinterpret_cast<const f32x4_t*>(p.rowvec + (size_t)(m / p.rowvec_div) * p.rowvec_ld + no);
        v += rv;
    }
    act_apply(v, p.act);
    if (p.residual) {
        const u32x2_t r = *reinterpret_cast<const u32x2_t*>(reinterpret_cast<const uint16_t*>(p.residual) + (size_t)m * p.ldr + no);
        const float rs = p.res_scale != 0.f ? p.res_scale : 1.f;
        v.x += rs * elem_lo(r.x); v.y += rs * elem_hi(r.x); v.z += rs * elem_lo(r.y); v.w += rs * elem_hi(r.y);
    }
    if (p.out_fp32) {
        *reinterpret_cast<f32x4_t*>(reinterpret_cast<float*>(p.out) + (size_t)m * p.ldo + no) = v;
    } else {
        u32x2_t o;
        o.x = pack_elem2(v.x, v.y); o.y = pack_elem2(v.z, v.w);
        *reinterpret_cast<u32x2_t*>(reinterpret_cast<uint16_t*>(p.out) + (size_t)m * p.ldo + no) = o;
    }
}

}  // namespace vmvg
