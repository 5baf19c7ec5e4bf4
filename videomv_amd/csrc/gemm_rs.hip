// gemm_rs.hip — ROW-STATIONARY implicit GEMM for the short-K linears of the transformer blocks (same contract as gemm.hip /
// vmv.h; K = 320 / 640 = the channel counts of the UNet's two large levels, and K = 512 = the init TemporalTransformer's 8 x 64 heads).
//
// Why: at K = C the tile kernels spend a tile's life outside their main loop.  A 256 x 128 tile of the K = 320 GEGLU is five
// 64-deep chunks: per chunk the CU's LDS-DMA path moves 48 KB (A + W) for 1 k cycles of MFMAs, the epilogue is as long as
// the loop, and the result (profiles/r2_ops_40x64.tsv) is 19-28 % of the MFMA peak at L0 with every unit half idle.  These
// GEMMs are also close to the HBM roofline (qkv: 315 MB for 75 GFLOP), so what counts is bytes through the CU per MAC.
// Here the ACTIVATIONS never enter LDS:
//   * a wave keeps RT x 16 rows of A — the whole K range — in registers (RT = 4, K = 320: 160 registers; loaded once,
//     fragment-shaped, straight from HBM / L2);
//   * a block of 8 waves (RT x 128 rows) streams the weight matrix through a three-stage LDS ring in 40-KB chunks
//     (64 W rows at K = 320) by LDS-DMA: per MAC 1/512 of a byte instead of 1/256 + 1/128, and the LDS port only serves W
//     fragments (one ds_read_b128 per RT MFMAs);
//   * K is complete inside the wave, so an output tile is FINISHED after K/32 MFMAs per row tile: there is no accumulator
//     array to drain, no tile epilogue — bias, GEGLU, residual and the store follow each pair of 16-column tiles while the
//     SIMD's other wave multiplies; two lane swaps (v_permlane16_swap) turn the MFMA's 4-channel lane slices into 16-byte
//     stores (64 B per row per instruction);
//   * a LayerNorm folded into the GEMM (vmv.h: colsum / ln_eps) is applied to the resident rows before the first MFMA:
//     two-pass statistics from the registers, x <- (x - mean) * rstd, then the plain product with W' = W diag(gamma) —
//     no statistics launch, no rowstat traffic, no colsum correction in the epilogue.
// One barrier per chunk (160 MFMAs per wave); the ring runs two chunks ahead.
// The ring, the MFMA pair, the LayerNorm of the resident rows and the store path are gemm_rs_common.h's, shared with gemm_ff / gemm_tqa / gemm_trs.
#include "gemm_rs_common.h"
#include <type_traits>

using namespace vmvg;

namespace {

template <int RT, int KS>
struct RsCfg : RsRing<KS> {
    using Ring = RsRing<KS>;
    static constexpr int BM = Ring::NW * RT * 16;              // rows per block
    static constexpr int MAX_COLS = 5120;                      // W rows one block walks (bias strip: 20 KB)
    static constexpr int TAB_BYTES = 2 * 2 * Ring::K * 4;      // folded GroupNorm: (scale | shift)[K] fp32 of the two stat groups a block can touch
    static constexpr int LDS_BYTES = Ring::STAGES * Ring::CHUNK_BYTES + MAX_COLS * 4 + TAB_BYTES;
    static_assert(LDS_BYTES <= 160 * 1024, "LDS budget");
};

constexpr int RS_GEGLU = 1, RS_LN = 2, RS_RES = 4, RS_GN = 8;

template <int RT, int KS, int MODE>
__global__ __launch_bounds__(512, 1) void gemm_rs_kernel(const VmvGemmParams p, const int tiles_m, const int nsplit, const int cols_per_split) {
    VMV_KERNEL_ENTER();
    using Cfg = RsCfg<RT, KS>;
    constexpr bool GEGLU = (MODE & RS_GEGLU) != 0, LN = (MODE & RS_LN) != 0, RES = (MODE & RS_RES) != 0, GN = (MODE & RS_GN) != 0;
    constexpr int RB = Cfg::RB, G = Cfg::G, P = Cfg::PIECES;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int frow = lane & 15, fgrp = lane >> 4;

    // ---- block -> (row tile, column split); XCD-aware bijection: the splits of one row tile run on one XCD (A comes from its L2)
    const int nblk = tiles_m * nsplit;
    const int logical = xcd_logical(blockIdx.x, nblk);
    const int mt = logical / nsplit, ns = logical - mt * nsplit;
    const int m_wave = mt * Cfg::BM + wave * (16 * RT);
    const int n_begin = ns * cols_per_split;
    const int ncols = (p.N - n_begin) < cols_per_split ? (p.N - n_begin) : cols_per_split;     // W rows of this block: k * CROWS (launcher)
    const int NC = ncols / Cfg::CROWS;

    // ---- the wave's RT x 16 rows of A, whole K range, straight into registers (rows >= M read as zero through the descriptor)
    const VmvGemmSeg& sg = p.seg[0];
    const __amdgpu_buffer_rsrc_t a_rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(sg.src), 0, (uint32_t)p.M * (uint32_t)sg.ld * 2u, SRD_FLAGS);
    u32x4_t a[RT][KS];
#pragma unroll
    for (int i = 0; i < RT; ++i) {
        const uint32_t vo = (uint32_t)((m_wave + 16 * i + frow) * sg.ld + 8 * fgrp) * 2u;
#pragma unroll
        for (int kk = 0; kk < KS; ++kk) a[i][kk] = __builtin_amdgcn_raw_buffer_load_b128(a_rsrc, vo + (uint32_t)(kk * 64), 0, 0);
    }

    // ---- loader: bias strip, then the W ring (gemm_rs_common.h: a chunk is CROWS whole rows of W, swizzled on the SOURCE address)
    float* bias_lds = reinterpret_cast<float*>(smem + Cfg::STAGES * Cfg::CHUNK_BYTES);
    {
        const __amdgpu_buffer_rsrc_t b_rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.bias), 0, p.bias ? (uint32_t)p.N * 4u : 0u, SRD_FLAGS);
        for (int q = wave; q * 256 < ncols; q += Cfg::NW)      // 256 floats per wave-instruction; columns >= N / no bias: zeros
            blds16(b_rsrc, reinterpret_cast<unsigned char*>(bias_lds) + q * 1024, (uint32_t)(n_begin + q * 256 + 4 * lane) * 4u, 0);
    }
    // folded GroupNorm (vmv.h: gn_table): a block's rows lie in at most two consecutive stat groups (gn_rows_per_stat >= BM); their
    // scale / shift rows — 2 x 2 x K floats, contiguous in the table — go to LDS behind the bias strip, before the W ring
    float* tab_lds = bias_lds + Cfg::MAX_COLS;
    int gn_first = 0;
    if constexpr (GN) {
        gn_first = (mt * Cfg::BM) / p.gn_rows_per_stat;
        const uint32_t nstat = (uint32_t)((p.M + p.gn_rows_per_stat - 1) / p.gn_rows_per_stat);
        const __amdgpu_buffer_rsrc_t t_rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.gn_table), 0, nstat * (uint32_t)(2 * Cfg::K * 4), SRD_FLAGS);
        for (int q = wave; q * 1024 < Cfg::TAB_BYTES; q += Cfg::NW)
            blds16(t_rsrc, reinterpret_cast<unsigned char*>(tab_lds) + q * 1024, (uint32_t)(gn_first * 2 * Cfg::K * 4 + q * 1024 + 16 * lane), 0);
    }
    const __amdgpu_buffer_rsrc_t w_rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p.W), 0, (uint32_t)p.N * (uint32_t)p.ktot * 2u, SRD_FLAGS);
    auto issue_chunk = [&](int c, int slot) {
        unsigned char* base = Cfg::wave_base(smem + slot * Cfg::CHUNK_BYTES, wave);
        const uint32_t so = (uint32_t)((n_begin + c * Cfg::CROWS) * p.ktot) * 2u;
        rs_issue_rows<Cfg>(w_rsrc, base, wave, lane, so, [&](const int r) { return r * p.ktot; });
    };
    const int pro = NC < Cfg::STAGES ? NC : Cfg::STAGES;
    for (int c = 0; c < pro; ++c) issue_chunk(c, c);

    // ---- folded GroupNorm: x <- elem(x * scale[c] + shift[c]) — the values vmv_groupnorm_apply would have stored — on the resident rows
    if constexpr (GN) {
        wait_vmcnt_rt(pro * P);                      // everything issued before the W ring has landed (in-order): my A rows, my table pieces
        __syncthreads();                             // ... and every wave's table pieces
        // per row tile the LDS address of its stat group's table (scalar select), per (row tile, k-step) 16 table values; the loop is
        // fenced per step and reads one step ahead: left to itself the scheduler hoists every step's reads (600 spilled registers)
        const float* tbase[RT];
#pragma unroll
        for (int i = 0; i < RT; ++i) {
            const int l = __builtin_amdgcn_readfirstlane((m_wave + 16 * i) / p.gn_rows_per_stat - gn_first);      // 0 or 1
            tbase[i] = tab_lds + (l ? 2 * Cfg::K : 0) + 8 * fgrp;
        }
        constexpr int GPF = 1, GNB = GPF + 1;        // table reads run GPF steps ahead (16 registers per step in flight; 2 measured the same)
        f32x4_t tv[GNB][4];
        int chain = 0;                               // always 0; ties each read to an earlier step's result (see the asm below)
        auto rd = [&](int idx, f32x4_t (&t)[4]) {
            const float* tb = tbase[idx / KS] + (idx % KS) * 32 + chain;
            t[0] = *reinterpret_cast<const f32x4_t*>(tb); t[1] = *reinterpret_cast<const f32x4_t*>(tb + 4);
            t[2] = *reinterpret_cast<const f32x4_t*>(tb + Cfg::K); t[3] = *reinterpret_cast<const f32x4_t*>(tb + Cfg::K + 4);
        };
#pragma unroll
        for (int idx = 0; idx < GPF; ++idx) rd(idx, tv[idx % GNB]);
#pragma unroll
        for (int idx = 0; idx < RT * KS; ++idx) {
            if (idx + GPF < RT * KS) rd(idx + GPF, tv[(idx + GPF) % GNB]);
            __builtin_amdgcn_sched_barrier(0);
            const f32x4_t sc0 = tv[idx % GNB][0], sc1 = tv[idx % GNB][1], sh0 = tv[idx % GNB][2], sh1 = tv[idx % GNB][3];
            u32x4_t v = a[idx / KS][idx % KS];
            v.x = pack_elem2(fmaf(elem_lo(v.x), sc0.x, sh0.x), fmaf(elem_hi(v.x), sc0.y, sh0.y));
            v.y = pack_elem2(fmaf(elem_lo(v.y), sc0.z, sh0.z), fmaf(elem_hi(v.y), sc0.w, sh0.w));
            v.z = pack_elem2(fmaf(elem_lo(v.z), sc1.x, sh1.x), fmaf(elem_hi(v.z), sc1.y, sh1.y));
            v.w = pack_elem2(fmaf(elem_lo(v.w), sc1.z, sh1.z), fmaf(elem_hi(v.w), sc1.w, sh1.w));
            a[idx / KS][idx % KS] = v;
            // (a fence for the optimiser, not only the scheduler: without a data dependency every step's table reads are issued up
            //  front — 640 live registers; the empty asm makes a later read's address "depend" on this step's result)
            asm volatile("" : "+v"(chain) : "v"(v.x), "v"(v.y), "v"(v.z), "v"(v.w));
            __builtin_amdgcn_sched_barrier(0);
        }
    }

    if constexpr (LN) rs_layernorm_rows(a, p.ln_eps);

    // ---- output / residual addressing: after the lane swaps a lane holds 8 consecutive channels of row frow:
    //      columns (fgrp & 1) * 16 + (fgrp >> 1) * 8 .. + 8 of the 32-column pair
    const int lanecol = (fgrp & 1) * 16 + (fgrp >> 1) * 8;
    const __amdgpu_buffer_rsrc_t out_rsrc = __builtin_amdgcn_make_buffer_rsrc(p.out, 0, SRD_RECORDS, SRD_FLAGS);
    const __amdgpu_buffer_rsrc_t res_rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p.residual), 0, SRD_RECORDS, SRD_FLAGS);
    const uint32_t ovo = (uint32_t)(frow * p.ldo + lanecol) * 2u;
    // GEGLU (one 16-column output tile per pair): the swap pairs two ROW tiles instead — lanes with even fgrp end up with 8
    // channels of row frow of tile i, odd fgrp with those of tile i + 1; columns (fgrp >> 1) * 8 .. + 8
    const uint32_t ovo_g = (uint32_t)((frow + 16 * (fgrp & 1)) * p.ldo + (fgrp >> 1) * 8) * 2u;
    const uint32_t rvo = (uint32_t)(frow * p.ldr + lanecol) * 2u;
    const float rs = p.res_scale != 0.f ? p.res_scale : 1.f;
    auto row_ok = [&](int i) { return m_wave + 16 * i + frow < p.M; };

    // ---- first chunk (and the bias strip, issued before it) visible to every wave
    if (pro >= 3) wait_vmcnt_rt(2 * P); else if (pro == 2) wait_vmcnt_rt(P); else wait_vmcnt_rt(0);
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");

    // fragment addressing (rs_frag_offsets written out: called from here it moves the register count of 28 instantiations, by up to + 27 — DESIGN.md)
    const int fsw = KS == 10 ? ((frow >> 1) & 7) : frow;      // swz() of this lane's fragment rows
    constexpr int NB = KS == 10 ? 2 : 4;
    int foff[Cfg::NB];
#pragma unroll
    for (int r = 0; r < NB; ++r) foff[r] = frow * RB + (fgrp ^ (fsw & 3)) * 16 + ((r ^ (fsw >> 2)) - r) * 64;
    // (the residual variant at 64 rows per wave has no registers left for a second W fragment set: it is HBM-bound anyway)
    constexpr int PFD = (RES && RT == 4) ? 0 : 1;      // W-fragment prefetch distance in k-steps
    auto mma_pair = [&](const unsigned char* sbase, const int q, f32x4_t (&c0)[RT], f32x4_t (&c1)[RT]) {
        rs_mma_pair<false, PFD, Cfg>(a, sbase, q, foff, c0, c1);
    };
    // residual of one pair in store layout, requested before the pair's MFMAs
    auto load_res = [&](const int ocol, u32x4_t (&rv)[RT]) {
#pragma unroll
        for (int i = 0; i < RT; ++i)
            rv[i] = __builtin_amdgcn_raw_buffer_load_b128(res_rsrc, row_ok(i) ? rvo : OOB, (uint32_t)((m_wave + 16 * i) * p.ldr + ocol) * 2u, 0);
    };
    auto store_pair = [&](const int ocol, const int i, u32x4_t o) {
        rs_store16(rs_swap16(o), out_rsrc, row_ok(i) ? ovo : OOB, (uint32_t)((m_wave + 16 * i) * p.ldo + ocol) * 2u);
    };

    // body b: W rows [64 b, 64 b + 64) of the block = two pairs; one chunk (G = 4) or two (G = 2)
    const int nbody = ncols / 64;
    int c = 0, slot = 0;
    auto chunk_end = [&](const int stores) { rs_ring_step<Cfg>(c, slot, NC, stores, issue_chunk); };
    for (int b = 0; b < nbody; ++b) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const unsigned char* sbase = smem + slot * Cfg::CHUNK_BYTES;
            const int q = G == 4 ? h : 0;                         // pair index inside the chunk
            const int nrel = 64 * b + 32 * h;                     // first W row of the pair, relative to n_begin
            const int ocol = GEGLU ? (n_begin + nrel) / 2 : n_begin + nrel;        // first output column of the pair
            f32x4_t c0[RT], c1[RT];
            u32x4_t rv[RT];
            if constexpr (RES) load_res(ocol, rv);
            mma_pair(sbase, q, c0, c1);
            const bool cend = G == 2 || h == 1;                   // last pair of its chunk (compile-time after unrolling)
            constexpr int SP = GEGLU ? RT / 2 : RT;               // store instructions per pair
            const f32x4_t b0 = *reinterpret_cast<const f32x4_t*>(bias_lds + nrel + 4 * fgrp);
            const f32x4_t b1 = *reinterpret_cast<const f32x4_t*>(bias_lds + nrel + 16 + 4 * fgrp);
            if constexpr (GEGLU) {
                u32x2_t hp[RT];
#pragma unroll
                for (int i = 0; i < RT; ++i) {
                    f32x4_t v = c0[i] + b0;
                    const f32x4_t gt = c1[i] + b1;
                    v.x *= gelu_erf_f(gt.x); v.y *= gelu_erf_f(gt.y); v.z *= gelu_erf_f(gt.z); v.w *= gelu_erf_f(gt.w);
                    hp[i].x = pack_elem2(v.x, v.y); hp[i].y = pack_elem2(v.z, v.w);
                    if (i & 1) {
                        const u32x4_t o = rs_swap16(u32x4_t{hp[i - 1].x, hp[i - 1].y, hp[i].x, hp[i].y});
                        const bool ok = m_wave + 16 * (i - 1 + (fgrp & 1)) + frow < p.M;
                        rs_store16(o, out_rsrc, ok ? ovo_g : OOB, (uint32_t)((m_wave + 16 * (i - 1)) * p.ldo + ocol) * 2u);
                    }
                    // one row tile at a time: left alone the scheduler interleaves all 16 GELUs of the pair for ILP
                    __builtin_amdgcn_sched_barrier(0);
                }
            } else {
#pragma unroll
                for (int i = 0; i < RT; ++i) {
                    f32x4_t v0 = c0[i] + b0, v1 = c1[i] + b1;
                    if constexpr (RES) {
                        const u32x4_t r = rs_swap16(rv[i]);   // store layout -> this lane's 4 channels of tile 2 q (x, y) and 2 q + 1 (z, w)
                        v0.x += rs * elem_lo(r.x); v0.y += rs * elem_hi(r.x); v0.z += rs * elem_lo(r.y); v0.w += rs * elem_hi(r.y);
                        v1.x += rs * elem_lo(r.z); v1.y += rs * elem_hi(r.z); v1.z += rs * elem_lo(r.w); v1.w += rs * elem_hi(r.w);
                    }
                    u32x4_t o;
                    o.x = pack_elem2(v0.x, v0.y); o.y = pack_elem2(v0.z, v0.w);
                    o.z = pack_elem2(v1.x, v1.y); o.w = pack_elem2(v1.z, v1.w);
                    store_pair(ocol, i, o);
                }
            }
            // chunk_end(n): n = this wave's stores issued since chunk c + 1's DMA went out (at the chunk_end two chunks ago); they and
            // chunk c + 2's DMA may stay in flight.  (The first version waited for all but the last chunk's stores: with the
            // write path of a store-heavy GEMM backed up that is a write round trip on the critical path of every chunk.)
            if (cend) chunk_end(c == 0 ? SP * (G / 2) : 2 * SP * (G / 2));
        }
    }
}

struct RsPlan { int rt, nsplit, cols; };

// rows per wave (RT) and column splits: fewest rounds x block time over the CUs; ties go to the larger row tile (fewer W bytes
// per MAC) and the smaller split
bool rs_plan(const VmvGemmParams& p, int force_rt, RsPlan& best, int ncu) {
    const int K = p.ktot;
    bool found = false;
    double best_cost = 0;
    for (int rt = 4; rt >= 2; rt -= 2) {
        if (force_rt && rt != force_rt) continue;
        if ((K == 640 || K == 512) && rt != 2) continue;
        const int bm = 128 * rt;
        const long tm = (p.M + bm - 1) / bm;
        for (int ns = 1; ns <= 8; ns *= 2) {
            if (p.N % (64 * ns)) continue;
            const int cols = p.N / ns;
            if (cols > 5120) continue;
            const long blocks = tm * ns;
            const long rounds = (blocks + ncu - 1) / ncu;
            // block time ~ rows x columns (+ the resident rows' load, which a split repeats)
            const double cost = (double)rounds * ((double)bm * cols + 24.0 * bm * K / 32.0);
            if (!found || cost < best_cost * 0.999) { found = true; best_cost = cost; best = RsPlan{rt, ns, cols}; }
        }
    }
    return found;
}

template <int RT, int KS, int MODE>
int launch_rs(const VmvGemmParams& p, const RsPlan& pl, hipStream_t st) {
    using Cfg = RsCfg<RT, KS>;
    const int tiles_m = (p.M + Cfg::BM - 1) / Cfg::BM;
    static std::atomic<unsigned long long> attr{0};      // one per template instantiation; set once per (kernel, device)
    if (const int rc_attr = vmv_lds_attr_once(attr, reinterpret_cast<const void*>(&gemm_rs_kernel<RT, KS, MODE>), Cfg::LDS_BYTES)) return rc_attr;
    VMV_LAUNCH((gemm_rs_kernel<RT, KS, MODE>), dim3(tiles_m * pl.nsplit), dim3(Cfg::NT), Cfg::LDS_BYTES, st, p, tiles_m, pl.nsplit, pl.cols);
    return vmv_launch_status();
}

template <int RT, int KS>
int launch_rs_mode(const VmvGemmParams& p, const RsPlan& pl, int mode, hipStream_t st) {
    switch (mode) {
        case 0: return launch_rs<RT, KS, 0>(p, pl, st);
        case RS_GEGLU: return launch_rs<RT, KS, RS_GEGLU>(p, pl, st);
        case RS_LN: return launch_rs<RT, KS, RS_LN>(p, pl, st);
        case RS_LN | RS_GEGLU: return launch_rs<RT, KS, RS_LN | RS_GEGLU>(p, pl, st);
        case RS_RES: return launch_rs<RT, KS, RS_RES>(p, pl, st);
        case RS_GN: return launch_rs<RT, KS, RS_GN>(p, pl, st);
        default: return VMV_GLDS_UNSUPPORTED;
    }
}

}  // namespace

// What the row-stationary kernel serves: ONE linear segment covering the whole K = 320 / 640 row, 16-bit staged output, bias /
// GEGLU / residual / folded LayerNorm with in-kernel statistics (colsum + ln_eps; a rowstat from a statistics pass is not
// needed and, with ln_eps given, ignored).
bool vmv_gemm_rs_supported(const VmvGemmParams& p) {
    if (p.nseg != 1 || p.seg[0].mode != VMV_SEG_LINEAR || p.seg[0].k != p.ktot) return false;
    if (p.ktot != 320 && p.ktot != 640 && p.ktot != 512) return false;
    if (p.ksplit > 1 || p.out_fp32 || p.rowvec || p.act != VMV_ACT_NONE || p.wgroup_rows != 0) return false;
    if (p.N % 64) return false;
    const bool geglu = p.epilogue == VMV_EPI_GEGLU;
    const bool ln = p.colsum != nullptr;
    if (ln && !(p.ln_eps > 0.f)) return false;
    if (ln && p.residual) return false;
    if (geglu && p.residual) return false;
    if (p.gn_table) {            // folded GroupNorm: the plain projection only (proj_in), stat groups of whole 16-row tiles, >= a block's rows
        if (ln || geglu || p.residual) return false;
        if (p.gn_rows_per_stat < 512 || (p.gn_rows_per_stat & 15) || (((uintptr_t)p.gn_table) & 15)) return false;
    }
    const int n_out = geglu ? p.N / 2 : p.N;
    if ((p.ldo & 7) || (n_out & 7) || !vmv_aligned16(p.out)) return false;
    if (p.residual && ((p.ldr & 7) || !vmv_aligned16(p.residual))) return false;
    if (!vmv_gemm_spans32(p, p.M + 512, 0, p.M + 512, p.M + 512)) return false;      // 32-bit byte offsets, a tile's rows past M included
    RsPlan pl;
    return rs_plan(p, 0, pl, 256);
}

// policy: the eligible linears with enough rows to fill the chip (the UNet's two large levels)
bool vmv_gemm_rs_preferred(const VmvGemmParams& p) {
    if (!vmv_gemm_rs_supported(p)) return false;
    RsPlan pl;
    if (!rs_plan(p, 0, pl, 256)) return false;
    const long blocks = (long)((p.M + 128 * pl.rt - 1) / (128 * pl.rt)) * pl.nsplit;
    return blocks >= 160;
}

int vmv_gemm_rs_launch(const VmvGemmParams& p, int tile, hipStream_t st) {
    if (!vmv_gemm_rs_supported(p)) return VMV_GLDS_UNSUPPORTED;
    RsPlan pl;
    const int force_rt = tile == VMV_TILE_RS512 ? 4 : tile == VMV_TILE_RS256 ? 2 : 0;
    if (!rs_plan(p, force_rt, pl, rs_ncu_whole_xcds())) return VMV_GLDS_UNSUPPORTED;
    const int mode = (p.epilogue == VMV_EPI_GEGLU ? RS_GEGLU : 0) | (p.colsum ? RS_LN : 0) | (p.residual ? RS_RES : 0) | (p.gn_table ? RS_GN : 0);
    if (p.ktot == 320) return pl.rt == 4 ? launch_rs_mode<4, 10>(p, pl, mode, st) : launch_rs_mode<2, 10>(p, pl, mode, st);
    if (p.ktot == 512) return launch_rs_mode<2, 16>(p, pl, mode, st);      // (the init TemporalTransformer: 8 heads x 64 on a 320-channel level)
    return launch_rs_mode<2, 20>(p, pl, mode, st);
}
