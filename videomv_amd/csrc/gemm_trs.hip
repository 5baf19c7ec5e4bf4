// gemm_trs.hip — ROW-STATIONARY temporal (3,1,1) convolution at C = 320 with the GroupNorm apply (+ SiLU) folded into the resident
// rows (same contract as gemm_tfr.hip / vmv.h; TemporalConvBlock_v2, tools/modules/unet/util.py:1357-1392: 4 x [GroupNorm over all
// frames -> SiLU -> Conv3d (3,1,1)]).
//
// Why.  On the 256 x 320 tile the first level's temporal convolution is a K = 960 GEMM of 30 chunks whose fill, epilogue and staged
// stores are ~30 % of a tile's life, A goes through LDS once per tap, and the norm's apply pass in front writes and re-reads the whole
// tensor only so that the LDS-DMA path can fetch normalised values.  But for a wave that holds ALL F frames of its pixels
//     out[f] = Y0[f - 1] + Y1[f] + Y2[f + 1],   Y_t = A W_t^T,
// i.e. three K = 320 products of the SAME resident rows — N' = 3 N columns, the shape of the first level's q | k | v linear, which
// gemm_rs.hip / gemm_tqa.hip run row-stationary — and the taps are a shift of the OUTPUTS along the frame axis, which is whole inside
// the wave: no halo, no border select.  The weight layout [N][tap][C] (ktot = 960) already is a [3 N][320] matrix with row 3 n + tap.
//   * A wave owns 48 rows = all F frames of PPW = 48 / F pixels, FRAME-major: tile row tr = 16 i + u -> frame tr / PPW, pixel
//     tr % PPW.  A frame step is then a uniform shift by PPW rows, and the missing tap of the first / last frame is the shift's own
//     zero fill.  Rows of pixels past the tensor are read as zeros and never stored; a shift never mixes pixels (tr % PPW is kept).
//   * The rows are loaded once per row tile straight into registers (rs_load_rows) and — folded form — normalised there:
//     elem(silu(x * scale + shift)) in fp32, the values vmv_groupnorm_apply stores, with each row's own sample's table row (the
//     tables of all samples, <= 8, sit in LDS behind the bias strip).
//   * W streams through the three-stage ring of 64-row chunks of gemm_rs_common.h by LDS-DMA; the DMA's source address orders the rows of a
//     64-channel group as (pair 0: tap 0, 1, 2), (pair 1: tap 0, 1, 2), 32 rows each — six halves = three chunks per item.
//   * Per 32-column pair: tap 0's product is shifted down by PPW rows into the output registers, tap 1's is added, tap 2's is shifted
//     up and added.  In the transposed-product layout a row is lane u of fragment i of a 16-lane group, so the shift is a DPP
//     row_shr / row_shl plus the carry from the neighbouring fragment (row_ror into the lanes the shift leaves): no LDS, no barrier.
//     Then bias, residual, v_permlane16_swap and 16-byte stores (rs_swap16 / rs_store16).
//   * Persistent blocks, one per CU, over contiguous, equally long ranges of (row tile, 64-channel group) items (gemm_tqa.hip); the
//     rows are re-loaded (and re-normalised) only where a range crosses a row-tile boundary.
#include "gemm_rs_common.h"
#include <cstdlib>
#include <type_traits>

using namespace vmvg;

bool vmv_gemm_tfr_preferred(const VmvGemmParams& p);            // gemm_tfr.hip

namespace {

using TrRing = RsRing<10>;                                  // chunk = 64 W rows of K = 320 = two (pair, tap) halves
constexpr int TR_RT = 3, TR_KS = TrRing::KS, TR_K = TrRing::K;
constexpr int TR_ROWS = 16 * TR_RT;                         // tile rows of a wave (F x pixels)
constexpr int TR_RB = TrRing::RB, TR_CHUNK = TrRing::CHUNK_BYTES, TR_STAGES = TrRing::STAGES;
constexpr int TR_MAXCOLS = 1280;                            // bias strip
constexpr int TR_MAXSAMP = 8;                               // samples whose norm tables fit behind it
constexpr int TR_TAB = TR_MAXSAMP * 2 * TR_K * 4;           // [sample][scale | shift][C] fp32: 20 KB (whole 1-KB DMA pieces)
constexpr int TR_OFF_BIAS = TR_STAGES * TR_CHUNK, TR_OFF_TAB = TR_OFF_BIAS + TR_MAXCOLS * 4;
constexpr int TR_LDS = TR_OFF_TAB + TR_TAB;
static_assert(TrRing::CROWS == 64 && (TR_TAB % 1024) == 0 && TR_LDS <= 160 * 1024, "chunk geometry");

// DPP move inside the 16-lane rows: a lane whose source lane lies outside its row keeps `old`
constexpr int DPP_ROW_SHL = 0x100, DPP_ROW_SHR = 0x110, DPP_ROW_ROR = 0x120;
template <int CTRL>
VMV_DEV float tr_dpp(float old, float v) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, old), __builtin_bit_cast(int, v), CTRL, 0xf, 0xf, false));
#else
    return old + v;
#endif
}
// o[tr] = y[tr - S] (tile rows tr = 16 i + lane u; rows < S: zero): lanes u >= S take lane u - S of their own fragment, lanes u < S
// lane u - S + 16 of the fragment below
template <int S>
VMV_DEV void tr_shift_down(const f32x4_t (&y)[TR_RT], f32x4_t (&o)[TR_RT]) {
#pragma unroll
    for (int i = 0; i < TR_RT; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float carry = i > 0 ? tr_dpp<DPP_ROW_ROR + S>(0.f, y[i - 1][r]) : 0.f;
            o[i][r] = tr_dpp<DPP_ROW_SHR + S>(carry, y[i][r]);
        }
}
// o[tr] += y[tr + S] (rows >= 48 - S: nothing): lanes u < 16 - S take lane u + S, the others lane u + S - 16 of the fragment above
template <int S>
VMV_DEV void tr_shift_up_add(const f32x4_t (&y)[TR_RT], f32x4_t (&o)[TR_RT]) {
#pragma unroll
    for (int i = 0; i < TR_RT; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float carry = i + 1 < TR_RT ? tr_dpp<DPP_ROW_ROR + 16 - S>(0.f, y[i + 1][r]) : 0.f;
            o[i][r] += tr_dpp<DPP_ROW_SHL + S>(carry, y[i][r]);
        }
}

// S = pixels per wave = 48 / F = the row shift of one frame step
template <bool GN, bool RES, int S>
__global__ __launch_bounds__(512, 1) void gemm_trs_kernel(const VmvGemmParams p, const int ntiles, const int ngroups, const int npix) {
    VMV_KERNEL_ENTER();
    constexpr int RT = TR_RT, KS = TR_KS, RB = TR_RB, P = TrRing::PIECES, PPW = S, F = TR_ROWS / S;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int frow = lane & 15, fgrp = lane >> 4;
    const int PX = p.P;

    // ---- persistent (row tile, 64-channel group) items, tile-major, in contiguous equally long ranges (gemm_tqa.hip)
    const int nblk = gridDim.x;
    const int logical = xcd_logical(blockIdx.x, nblk);
    const long nitems = (long)ntiles * ngroups;
    const int i0 = (int)(((long)logical * nitems) / nblk), i1 = (int)(((long)(logical + 1) * nitems) / nblk);
    const int nit = i1 - i0;                                    // >= 1 (the grid never exceeds the item count)

    // ---- the wave's 48 tile rows: tile row tr = 16 i + frow -> frame tr / PPW, pixel gp0 + tr % PPW -> global row (b F + f) P + pp
    const VmvGemmSeg& sg = p.seg[0];
    const int lanecol = (fgrp & 1) * 16 + (fgrp >> 1) * 8;      // after the lane swaps: this lane's 8 consecutive columns of a 32-column pair
    int mrow[RT];                                               // global row of tile row 16 i + frow, -1 = outside the tensor
    uint32_t tabo[RT];
    const __amdgpu_buffer_rsrc_t a_rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(sg.src), 0, (uint32_t)p.M * (uint32_t)sg.ld * 2u, SRD_FLAGS);
    u32x4_t a[RT][KS];
    auto load_tile = [&](const int tile) __attribute__((always_inline)) {      // frame-major rows of row tile `tile`
        const int gp0 = (tile * TrRing::NW + wave) * PPW;          // first (sample, pixel) index of this wave
        rs_load_rows(a, a_rsrc, sg.ld, gp0, frow, fgrp, F, PX, npix, [&](const int tr, int& f, int& px) { f = tr / PPW; px = tr - f * PPW; },
                     [&](const int i, const bool ok, const int b, const long m, const int) {
                         mrow[i] = ok ? (int)m : -1;
                         tabo[i] = (uint32_t)(TR_OFF_TAB + ((ok ? b : 0) * 2 * TR_K + 8 * fgrp) * 4);      // this row's sample's table, this lane's k-slice
                     });
    };
    int cur_tile = i0 / ngroups;
    load_tile(cur_tile);

    // ---- bias strip, the norm tables of every sample, then the W ring
    float* bias_lds = reinterpret_cast<float*>(smem + TR_OFF_BIAS);
    {
        const __amdgpu_buffer_rsrc_t b_rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.bias), 0, p.bias ? (uint32_t)p.N * 4u : 0u, SRD_FLAGS);
        for (int q = wave; q * 256 < TR_MAXCOLS; q += TrRing::NW)    // (columns >= N / no bias: zeros)
            blds16(b_rsrc, reinterpret_cast<unsigned char*>(bias_lds) + q * 1024, (uint32_t)(q * 256 + 4 * lane) * 4u, 0);
    }
    if constexpr (GN) {
        const uint32_t tbytes = (uint32_t)(p.M / (F * PX)) * (uint32_t)(2 * TR_K * 4);      // <= TR_TAB (launcher)
        const __amdgpu_buffer_rsrc_t t_rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.gn_table), 0, tbytes, SRD_FLAGS);
        for (int q = wave; q * 1024 < (int)tbytes; q += TrRing::NW)
            blds16(t_rsrc, smem + TR_OFF_TAB + q * 1024, (uint32_t)(q * 1024 + 16 * lane), 0);
    }
    const __amdgpu_buffer_rsrc_t w_rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p.W), 0, (uint32_t)p.N * (uint32_t)p.ktot * 2u, SRD_FLAGS);
    // chunk c of the block = halves 2 cc, 2 cc + 1 (cc = c % 3) of item i0 + c / 3; half hh = (pair hh / 3, tap hh % 3): chunk row r
    // is W row (n0 + 32 pair + (r & 31), tap) — channels >= N read as zeros through the descriptor
    auto issue_chunk = [&](int c, int slot) {
        unsigned char* base = TrRing::wave_base(smem + slot * TR_CHUNK, wave);
        const int it = c / 3, cc = c - 3 * it;
        const int n0 = 64 * ((i0 + it) % ngroups);
        rs_issue_rows<TrRing>(w_rsrc, base, wave, lane, 0, [&](const int r) {
            const int hh = 2 * cc + (r >> 5);
            const int pr = hh >= 3 ? 1 : 0, tp = hh - 3 * pr;
            const int n = n0 + 32 * pr + (r & 31);
            return n * p.ktot + tp * TR_K;
        });
    };
    const int NC = 3 * nit;
    for (int c = 0; c < TR_STAGES; ++c) issue_chunk(c, c);       // (NC >= 3 always)

    // ---- folded GroupNorm (+ SiLU) on the resident rows: x <- elem(silu(x * scale[c] + shift[c])), the values vmv_groupnorm_apply
    //      would have stored.  The loop is fenced per (row fragment, k-step) and reads one step ahead: left to itself the scheduler hoists
    //      every step's reads (600 spilled registers).  (gemm_rs.hip's proj_in fold is the same loop without SiLU, packing per dword.)
    const bool silu = p.gn_silu != 0;
    auto fold_rows = [&]() __attribute__((always_inline)) {
        if constexpr (GN) {
            f32x4_t tv[2][4];
            int chain = 0;                               // always 0; ties each read to an earlier step's result (the asm below)
            auto rd = [&](int idx, f32x4_t (&t)[4]) {
                const float* tb = reinterpret_cast<const float*>(smem + tabo[idx / KS]) + (idx % KS) * 32 + chain;
                t[0] = *reinterpret_cast<const f32x4_t*>(tb); t[1] = *reinterpret_cast<const f32x4_t*>(tb + 4);
                t[2] = *reinterpret_cast<const f32x4_t*>(tb + TR_K); t[3] = *reinterpret_cast<const f32x4_t*>(tb + TR_K + 4);
            };
            rd(0, tv[0]);
#pragma unroll
            for (int idx = 0; idx < RT * KS; ++idx) {
                if (idx + 1 < RT * KS) rd(idx + 1, tv[(idx + 1) & 1]);
                __builtin_amdgcn_sched_barrier(0);
                const f32x4_t sc0 = tv[idx & 1][0], sc1 = tv[idx & 1][1], sh0 = tv[idx & 1][2], sh1 = tv[idx & 1][3];
                u32x4_t v = a[idx / KS][idx % KS];
                float x0 = fmaf(elem_lo(v.x), sc0.x, sh0.x), x1 = fmaf(elem_hi(v.x), sc0.y, sh0.y);
                float x2 = fmaf(elem_lo(v.y), sc0.z, sh0.z), x3 = fmaf(elem_hi(v.y), sc0.w, sh0.w);
                float x4 = fmaf(elem_lo(v.z), sc1.x, sh1.x), x5 = fmaf(elem_hi(v.z), sc1.y, sh1.y);
                float x6 = fmaf(elem_lo(v.w), sc1.z, sh1.z), x7 = fmaf(elem_hi(v.w), sc1.w, sh1.w);
                if (silu) {
                    x0 = silu_f(x0); x1 = silu_f(x1); x2 = silu_f(x2); x3 = silu_f(x3);
                    x4 = silu_f(x4); x5 = silu_f(x5); x6 = silu_f(x6); x7 = silu_f(x7);
                }
                v.x = pack_elem2(x0, x1); v.y = pack_elem2(x2, x3); v.z = pack_elem2(x4, x5); v.w = pack_elem2(x6, x7);
                a[idx / KS][idx % KS] = v;
                // (a fence for the optimiser, not only the scheduler: without a data dependency every step's table reads are issued up
                //  front — 640 live registers; the empty asm makes a later read's address "depend" on this step's result)
                asm volatile("" : "+v"(chain) : "v"(v.x), "v"(v.y), "v"(v.z), "v"(v.w));
                __builtin_amdgcn_sched_barrier(0);
            }
        }
    };
    if constexpr (GN) {
        wait_vmcnt_rt(TR_STAGES * P);                // everything issued before the W ring has landed (in-order): my rows, my table pieces
        __syncthreads();                             // ... and every wave's table pieces
    }
    fold_rows();

    const __amdgpu_buffer_rsrc_t out_rsrc = __builtin_amdgcn_make_buffer_rsrc(p.out, 0, SRD_RECORDS, SRD_FLAGS);
    const __amdgpu_buffer_rsrc_t res_rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p.residual), 0, SRD_RECORDS, SRD_FLAGS);
    const float rs = p.res_scale != 0.f ? p.res_scale : 1.f;

    // ---- first chunk (and the bias strip, issued before it) visible to every wave
    wait_vmcnt_rt(2 * P);
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");

    // (rs_frag_offsets written out: called from here it costs 16 of the 24 instantiations 2-6 registers — DESIGN.md)
    const int fsw = (frow >> 1) & 7;
    int foff[2];
#pragma unroll
    for (int r = 0; r < 2; ++r) foff[r] = frow * RB + (fgrp ^ (fsw & 3)) * 16 + ((r ^ (fsw >> 2)) - r) * 64;
    // one half = two 16-row W tiles (one tap of a 32-channel pair) against the resident rows, transposed product (c: row frow, channels
    // 4 fgrp + r of the tile)
    auto mma_pair = [&](const unsigned char* sbase, const int q, f32x4_t (&c0)[RT], f32x4_t (&c1)[RT]) {
        rs_mma_pair<false, 1, TrRing>(a, sbase, q, foff, c0, c1);
    };

    int c = 0, slot = 0;
    // chunk c consumed: chunk c + 1 landed for every wave, slot of chunk c refilled with chunk c + 3.  `extra` = a lower bound of this
    // wave's stores / residual loads issued behind chunk c + 1's DMA (the previous and the current chunk's): they and chunk c + 2's DMA
    // may stay in flight.
    auto chunk_end = [&](const int extra) { rs_ring_step<TrRing>(c, slot, NC, extra, issue_chunk); };
    // vector-memory operations of this wave per chunk of an item: chunk 0 none; chunk 1 the residual loads and stores of pair 0; chunk 2
    // those of pair 1
    constexpr int NVM = RES ? 2 * RT : RT;

    for (int it = 0; it < nit; ++it) {
        const int tile = (i0 + it) / ngroups, g = (i0 + it) - tile * ngroups;
        if (tile != cur_tile) {         // the range crossed into the next row tile: new rows (every MFMA on the old ones has issued; the
            cur_tile = tile;            // compiler's own waits cover the loads; the ring's DMAs in flight are untouched)
            load_tile(tile);
            fold_rows();
        }
        f32x4_t o0[RT], o1[RT];
#pragma unroll
        for (int h = 0; h < 6; ++h) {
            const int pr = h / 3, tap = h - 3 * pr;
            const int ocol = 64 * g + 32 * pr;                      // first output column of the pair
            const unsigned char* sbase = smem + slot * TR_CHUNK;
            const bool col_ok = ocol < p.N;                         // (N % 64 == 32: the last group's second pair does not exist)
            u32x4_t rv[RT];
            if constexpr (RES) {                                    // residual of the pair in store layout, requested before the last tap's MFMAs
                if (tap == 2) {
#pragma unroll
                    for (int i = 0; i < RT; ++i)
                        rv[i] = __builtin_amdgcn_raw_buffer_load_b128(res_rsrc, col_ok && mrow[i] >= 0 ? (uint32_t)(mrow[i] * p.ldr + lanecol) * 2u : OOB, (uint32_t)ocol * 2u, 0);
                }
            }
            f32x4_t c0[RT], c1[RT];
            mma_pair(sbase, h & 1, c0, c1);
            if (tap == 0) {                                         // W tap 0 multiplies frame f - 1
                tr_shift_down<S>(c0, o0); tr_shift_down<S>(c1, o1);
            } else if (tap == 1) {
#pragma unroll
                for (int i = 0; i < RT; ++i) { o0[i] += c0[i]; o1[i] += c1[i]; }
            } else {                                                // W tap 2 multiplies frame f + 1
                tr_shift_up_add<S>(c0, o0); tr_shift_up_add<S>(c1, o1);
                const f32x4_t b0 = *reinterpret_cast<const f32x4_t*>(bias_lds + ocol + 4 * fgrp);
                const f32x4_t b1 = *reinterpret_cast<const f32x4_t*>(bias_lds + ocol + 16 + 4 * fgrp);
#pragma unroll
                for (int i = 0; i < RT; ++i) {
                    f32x4_t v0 = o0[i] + b0, v1 = o1[i] + b1;
                    act_apply(v0, p.act); act_apply(v1, p.act);
                    if constexpr (RES) {
                        const u32x4_t r = rs_swap16(rv[i]);     // store layout -> this lane's 4 channels of the two tiles
                        v0.x += rs * elem_lo(r.x); v0.y += rs * elem_hi(r.x); v0.z += rs * elem_lo(r.y); v0.w += rs * elem_hi(r.y);
                        v1.x += rs * elem_lo(r.z); v1.y += rs * elem_hi(r.z); v1.z += rs * elem_lo(r.w); v1.w += rs * elem_hi(r.w);
                    }
                    const u32x4_t ov = u32x4_t{pack_elem2(v0.x, v0.y), pack_elem2(v0.z, v0.w), pack_elem2(v1.x, v1.y), pack_elem2(v1.z, v1.w)};
                    rs_store16(rs_swap16(ov), out_rsrc, col_ok && mrow[i] >= 0 ? (uint32_t)(mrow[i] * p.ldo + lanecol) * 2u : OOB, (uint32_t)ocol * 2u);
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
            if (h == 1) chunk_end(it > 0 ? NVM : 0);                        // chunk 0 of the item (+ the previous item's chunk 2)
            else if (h == 3) chunk_end(NVM);                                // chunk 1 (+ chunk 0)
            else if (h == 5) chunk_end(2 * NVM);                            // chunk 2 (+ chunk 1)
        }
    }
}

long trs_items(const VmvGemmParams& p) {
    return (long)rs_pixel_tiles(p, TR_ROWS).ntiles * ((p.N + 63) / 64);
}

}  // namespace

// host logic: can the row-stationary temporal kernel serve *p at all (forced tile or policy)?
bool vmv_gemm_trs_supported(const VmvGemmParams& p) {
    if (p.nseg != 3 || (p.F != 12 && p.F != 16 && p.F != 24) || p.P <= 0) return false;
    const VmvGemmSeg& s0 = p.seg[0];
    for (int i = 0; i < 3; ++i) {
        const VmvGemmSeg& sg = p.seg[i];
        if (sg.mode != VMV_SEG_TEMPORAL || sg.d0 != i - 1 || sg.src != s0.src || sg.ld != s0.ld || sg.k != s0.k) return false;
    }
    if (s0.k != TR_K || p.ktot != 3 * TR_K || (p.N % 32) || p.N > TR_MAXCOLS) return false;
    if ((long)p.M % ((long)p.F * p.P)) return false;
    if (p.epilogue != VMV_EPI_NONE || p.rowvec || p.rowstat || p.colsum || p.ln_eps > 0.f || p.wgroup_rows || p.ksplit > 1 || p.out_fp32 || p.phased) return false;
    if ((p.ldo & 7) || !vmv_aligned16(p.out) || (p.residual && ((p.ldr & 7) || !vmv_aligned16(p.residual)))) return false;
    if (p.gn_table && (p.gn_rows_per_stat != p.F * p.P || !vmv_aligned16(p.gn_table) || p.M / ((long)p.F * p.P) > TR_MAXSAMP)) return false;
    if (p.gn_silu && !p.gn_table) return false;
    if (!vmv_gemm_spans32(p, p.M, 64, p.M, p.M)) return false;      // 32-bit byte offsets: the source, W with a group's rows past N, output, residual
    return true;
}

// policy: the FOLDED form (gn_table) of the C = 320 temporal convolution once the (row tile, 64-channel group) items give every other CU
// a block; the frame-resident kernel keeps the shapes its own policy takes (24 x 32 x 32).  VMV_TRS_MIN_ITEMS: tests reach the kernel at
// small shapes.
bool vmv_gemm_trs_preferred(const VmvGemmParams& p) {
    if (!p.gn_table || !vmv_gemm_trs_supported(p) || vmv_gemm_tfr_preferred(p)) return false;
    const char* e = getenv("VMV_TRS_MIN_ITEMS");       // (read at every call, as VMV_UP4_MIN_ROWS: reached only by folded C = 320 temporal convolutions)
    return trs_items(p) >= (e ? atol(e) : 128);
}

// max_blocks > 0 caps the grid (tests: item ranges that cross row tiles at small shapes)
int vmv_gemm_trs_launch(const VmvGemmParams& p, int max_blocks, hipStream_t st) {
    if (!vmv_gemm_trs_supported(p)) return VMV_GLDS_UNSUPPORTED;
    const int npix = rs_pixel_tiles(p, TR_ROWS).npix, ntiles = rs_pixel_tiles(p, TR_ROWS).ntiles;
    const int ngroups = (p.N + 63) / 64;
    const long nitems = trs_items(p);
    int nblk = (int)(nitems < rs_ncu_whole_xcds() ? nitems : rs_ncu_whole_xcds());
    if (max_blocks > 0 && nblk > max_blocks) nblk = max_blocks;
    const bool gn = p.gn_table != nullptr, res = p.residual != nullptr;
#define TR_LAUNCH1(GNV, RESV, SV)                                                                                                               \
    do {                                                                                                                                 \
        static std::atomic<unsigned long long> attr{0};                                                                                  \
        if (const int rc = vmv_lds_attr_once(attr, reinterpret_cast<const void*>(&gemm_trs_kernel<GNV, RESV, SV>), TR_LDS)) return rc;         \
        VMV_LAUNCH((gemm_trs_kernel<GNV, RESV, SV>), dim3(nblk), dim3(TrRing::NT), TR_LDS, st, p, ntiles, ngroups, npix);                           \
    } while (0)
#define TR_LAUNCH(SV)                                                                                                                    \
    do {                                                                                                                                 \
        if (gn) { if (res) TR_LAUNCH1(true, true, SV); else TR_LAUNCH1(true, false, SV); }                                               \
        else { if (res) TR_LAUNCH1(false, true, SV); else TR_LAUNCH1(false, false, SV); }                                                \
    } while (0)
    if (p.F == 24) TR_LAUNCH(2); else if (p.F == 16) TR_LAUNCH(3); else TR_LAUNCH(4);
#undef TR_LAUNCH
#undef TR_LAUNCH1
    return vmv_launch_status();
}
