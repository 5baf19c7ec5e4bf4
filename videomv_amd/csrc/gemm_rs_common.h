// gemm_rs_common.h — shared by the ROW-STATIONARY kernels (gemm_rs / gemm_ff / gemm_tqa / gemm_trs): a wave keeps its activation rows,
// the whole K range, in registers as MFMA fragments a[RT][KS] (lane (frow = lane & 15, fgrp = lane >> 4) holds k-slice 4 kk + fgrp of
// row 16 i + frow) and the block streams W through an LDS ring of whole-row chunks by LDS-DMA.  One definition each of the ring
// geometry, the DMA issue and ring step, the fragment addressing and MFMA pair, the LayerNorm of the resident rows, the lane swap and
// store path with their hardware-hazard workarounds, and the host arithmetic of the persistent kernels.  Every piece compiles to
// the instructions its per-kernel copies compiled to, or to a measured equivalent ("Shared parts"; what is NOT shared
// is listed there).  How the functions take their arguments is part of that: rs_issue_rows, rs_mma_pair, rs_ring_step and rs_load_rows
// are called from the kernels' lambdas and take what those lambdas captured BY REFERENCE (rs_issue_rows and rs_mma_pair are also left
// to the ordinary inliner, not VMV_DEV): by value, or force-inlined before the lambda is optimised, the same arithmetic comes out in
// another issue order.  Check any change here against the parent's device assembly (hipcc --cuda-device-only -S), per element type.
#pragma once
#include "gemm_glds_common.h"

namespace vmvg {

// ---- ring geometry: chunks of whole W rows (K = 32 KS elements), 8 waves, three stages
template <int KS_>
struct RsRing {
    static constexpr int KS = KS_, NW = 8, NT = 512;
    static constexpr int K = KS * 32;
    static constexpr int RB = K * 2;                           // bytes per W row
    static constexpr int SPR = RB / 16;                        // 16-byte slots per W row (40 / 80)
    static constexpr int CHUNK_BYTES = KS == 16 ? 32768 : 40960;   // whole W rows: 64 x 640 B, 32 x 1280 B, 32 x 1024 B (K = 512: round 6)
    static constexpr int CROWS = CHUNK_BYTES / RB;             // W rows per chunk (64 / 32)
    static constexpr int G = CROWS / 16;                       // 16-row W tiles per chunk (4 / 2)
    static constexpr int STAGES = 3;
    static constexpr int PIECES = CHUNK_BYTES / 1024 / NW;     // LDS-DMA wave-instructions per wave per chunk (5; 4 at K = 512)
    static constexpr int NB = KS == 10 ? 2 : 4;                // fragment lane offsets (rs_frag_offsets)
    static_assert(CROWS * RB == CHUNK_BYTES && (G == 2 || G == 4) && PIECES * NW * 1024 == CHUNK_BYTES, "chunk geometry");
    // LDS position (row r, 16-byte slot s') holds k-slot s' ^ swz(r) of that row, applied to the SOURCE address (the image of a DMA is
    // lane-linear): with 640-byte rows the 16 rows of a fragment alternate between the two halves of the 256-byte bank row, so
    // swz = (r >> 1) & 7 spreads them over all 16 16-byte units; with 1280-byte (1024-byte) rows every row starts on the same bank,
    // swz = r & 15.  Both are conflict-free for ds_read_b128's non-contiguous 16-lane groups (rows {0-3, 12-15} with k-slot f, rows
    // {4-11} with f ^ 1).
    VMV_DEV static constexpr int swz(const int r) { return KS == 10 ? ((r >> 1) & 7) : (r & 15); }
    VMV_DEV static unsigned char* wave_base(unsigned char* slot_base, const int wave) { return slot_base + wave * (PIECES * 1024); }
};

// ---- DMA issue: CROWS x K W rows into a ring slot; wave w fills bytes [1024 P w, 1024 P (w + 1)) of it, from `base` =
//      Ring::wave_base(slot's address, w), with P wave-instructions.  row_off(r) = element offset of chunk row r's source row behind `soff` bytes (rows past the descriptor: zeros).
//      (the P source offsets are recomputed per chunk — ~30 VALU operations per 160+ MFMAs — instead of living in P registers next
//       to 160 of resident rows; the empty asm keeps the compiler from hoisting them out of the loop again)
template <class Ring, class RowOff>
__device__ inline void rs_issue_rows(const __amdgpu_buffer_rsrc_t& w_rsrc, unsigned char* const& base, const int& wave, const int& lane, const uint32_t& soff, const RowOff& row_off) {
    constexpr int P = Ring::PIECES;
    int ln = lane;
    asm volatile("" : "+v"(ln));
#pragma unroll
    for (int q = 0; q < P; ++q) {
        const int u = wave * (P * 64) + q * 64 + ln;
        const int r = u / Ring::SPR, s = u - r * Ring::SPR;
        const int sw = Ring::swz(r);
        blds16(w_rsrc, base + q * 1024, (uint32_t)(row_off(r) + (s ^ sw) * 8) * 2u, soff);
    }
}

// ---- ring step: chunk c of NC consumed.  Chunk c + 1 has landed (mine: everything issued after its DMA — chunk c + 2's DMA and
//      `extra` vector-memory operations of this wave, a lower bound — may stay in flight), the barrier makes it visible and says every
//      wave is done with slot `slot`, which then takes chunk c + STAGES: issue(c + STAGES, slot).
template <class Ring, class Issue>
VMV_DEV void rs_ring_step(int& c, int& slot, const int& NC, const int extra, const Issue& issue) {
    if (c + 1 < NC) {
        wait_vmcnt_rt((c + 2 < NC ? Ring::PIECES : 0) + extra);
        __builtin_amdgcn_s_waitcnt(0xc07f);
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        if (c + Ring::STAGES < NC) issue(c + Ring::STAGES, slot);
    }
    ++c;
    slot = slot + 1 == Ring::STAGES ? 0 : slot + 1;
}

// ---- fragment addressing: this lane's rows 16 j + frow have swz = fsw (lane constant); k-slot (4 kk + fgrp) ^ fsw =
//      4 (kk ^ (fsw >> 2)) + (fgrp ^ (fsw & 3)), so with NB = 2 (4) lane offsets, one per kk mod NB, every read is base + 64 kk
template <class Ring>
VMV_DEV void rs_frag_offsets(const int frow, const int fgrp, int (&foff)[Ring::NB]) {
    const int fsw = Ring::swz(frow);
#pragma unroll
    for (int r = 0; r < Ring::NB; ++r) foff[r] = frow * Ring::RB + (fgrp ^ (fsw & 3)) * 16 + ((r ^ (fsw >> 2)) - r) * 64;
}

// ---- one pair q of 16-row W tiles of the chunk at `sbase` against the resident rows.  SWAP = false: transposed product (c: row frow,
//      channels 4 fgrp + r of the tile); SWAP = true: plain product (c: rows 4 fgrp + r, channel frow of the tile).
//      W fragments of k-step kk + PFD are requested before the MFMAs of k-step kk (the order is pinned: left alone the compiler
//      issues each pair of reads right in front of its MFMAs and the matrix pipe waits out the LDS latency 10 times per pair;
//      ablation on the GPU: with the reads removed the kernel runs 36-47 % faster, i.e. one k-step of cover — 8 MFMAs = 128
//      cycles at 64 rows per wave, 64 cycles at 32 — is less than the loaded LDS latency).  PFD = 0: no second fragment set.
template <bool SWAP, int PFD, class Ring, int RT>
__device__ inline void rs_mma_pair(const u32x4_t (&a)[RT][Ring::KS], const unsigned char* const& sbase, const int& q, const int (&foff)[Ring::NB], f32x4_t (&c0)[RT],
                         f32x4_t (&c1)[RT]) {
    constexpr int KS = Ring::KS, RB = Ring::RB, NB = Ring::NB, NBUF = PFD + 1;
    const unsigned char* tb[NB];
#pragma unroll
    for (int r = 0; r < NB; ++r) tb[r] = sbase + 32 * q * RB + foff[r];
#pragma unroll
    for (int i = 0; i < RT; ++i) { c0[i] = f32x4_t{0.f, 0.f, 0.f, 0.f}; c1[i] = f32x4_t{0.f, 0.f, 0.f, 0.f}; }
    u32x4_t w0[NBUF], w1[NBUF];
    auto rd = [&](const int kk, u32x4_t& x0, u32x4_t& x1) __attribute__((always_inline)) {
        const unsigned char* t = tb[kk & (NB - 1)] + 64 * kk;
        x0 = *reinterpret_cast<const u32x4_t*>(t);
        x1 = *reinterpret_cast<const u32x4_t*>(t + 16 * RB);
    };
#pragma unroll
    for (int kk = 0; kk < PFD; ++kk) rd(kk, w0[kk % NBUF], w1[kk % NBUF]);
#pragma unroll
    for (int kk = 0; kk < KS; ++kk) {
        const int cur = kk % NBUF;
        if (kk + PFD < KS) rd(kk + PFD, w0[(kk + PFD) % NBUF], w1[(kk + PFD) % NBUF]);
        if constexpr (PFD > 0) __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int i = 0; i < RT; ++i) {
            if constexpr (SWAP) {
                c0[i] = VMV_MFMA16(__builtin_bit_cast(elem8_t, a[i][kk]), __builtin_bit_cast(elem8_t, w0[cur]), c0[i], 0, 0, 0);
                c1[i] = VMV_MFMA16(__builtin_bit_cast(elem8_t, a[i][kk]), __builtin_bit_cast(elem8_t, w1[cur]), c1[i], 0, 0, 0);
            } else {
                c0[i] = VMV_MFMA16(__builtin_bit_cast(elem8_t, w0[cur]), __builtin_bit_cast(elem8_t, a[i][kk]), c0[i], 0, 0, 0);
                c1[i] = VMV_MFMA16(__builtin_bit_cast(elem8_t, w1[cur]), __builtin_bit_cast(elem8_t, a[i][kk]), c1[i], 0, 0, 0);
            }
        }
        if constexpr (PFD > 0) __builtin_amdgcn_sched_barrier(0);
    }
}

// ---- LayerNorm of the resident rows (two-pass, fp32): lanes frow, frow + 16, + 32, + 48 hold the four k-quarters of a row;
//      x <- (x - mean) * rstd, the plain product with W' = W diag(gamma) follows
template <int RT, int KS>
VMV_DEV void rs_layernorm_rows(u32x4_t (&a)[RT][KS], const float eps) {
    const float inv_k = 1.0f / (float)(32 * KS);
#pragma unroll
    for (int i = 0; i < RT; ++i) {
        float s1 = 0.f;
#pragma unroll
        for (int kk = 0; kk < KS; ++kk) {
            elem_dot2c(s1, a[i][kk].x, VMV_ELEM_ONE2); elem_dot2c(s1, a[i][kk].y, VMV_ELEM_ONE2);
            elem_dot2c(s1, a[i][kk].z, VMV_ELEM_ONE2); elem_dot2c(s1, a[i][kk].w, VMV_ELEM_ONE2);
        }
        // (v_dot2c is a DOT-pipe instruction: on gfx940+ its result needs 3-4 wait states before a different VALU reads it,
        //  and hipcc pads nothing for an instruction it only sees as inline asm — without this the next v_mov picked up a
        //  stale partial sum: means off by ~1e-2 sigma on the first GPU run)
        asm volatile("s_nop 4" : "+v"(s1));
        const float mean = xor16_32_sum(s1) * inv_k;
        float s2 = 0.f;
#pragma unroll
        for (int kk = 0; kk < KS; ++kk) {
            const uint32_t w4[4] = {a[i][kk].x, a[i][kk].y, a[i][kk].z, a[i][kk].w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float d0 = elem_lo(w4[e]) - mean, d1 = elem_hi(w4[e]) - mean;
                s2 = fmaf(d0, d0, s2); s2 = fmaf(d1, d1, s2);
            }
        }
        const float rstd = __builtin_amdgcn_rsqf(xor16_32_sum(s2) * inv_k + eps);
        const float nm = -mean * rstd;
        // (the normalisation pass unpacks the same registers as the variance pass: left visible, the compiler keeps the 80
        //  unpacked fp32 values of the row tile alive in between — the bf16 build, whose unpack is a shift, spilled 300
        //  registers that way — so the packed registers are made opaque here)
#pragma unroll
        for (int kk = 0; kk < KS; ++kk) asm volatile("" : "+v"(a[i][kk].x), "+v"(a[i][kk].y), "+v"(a[i][kk].z), "+v"(a[i][kk].w));
#pragma unroll
        for (int kk = 0; kk < KS; ++kk) {
            a[i][kk].x = pack_elem2(fmaf(elem_lo(a[i][kk].x), rstd, nm), fmaf(elem_hi(a[i][kk].x), rstd, nm));
            a[i][kk].y = pack_elem2(fmaf(elem_lo(a[i][kk].y), rstd, nm), fmaf(elem_hi(a[i][kk].y), rstd, nm));
            a[i][kk].z = pack_elem2(fmaf(elem_lo(a[i][kk].z), rstd, nm), fmaf(elem_hi(a[i][kk].z), rstd, nm));
            a[i][kk].w = pack_elem2(fmaf(elem_lo(a[i][kk].w), rstd, nm), fmaf(elem_hi(a[i][kk].w), rstd, nm));
        }
    }
}
template <int KS>
VMV_DEV void rs_layernorm_rows(u32x4_t (&a)[KS], const float eps) { rs_layernorm_rows<1, KS>(reinterpret_cast<u32x4_t (&)[1][KS]>(a), eps); }

// ---- rows of a persistent kernel's row tile into the registers: 8 waves x 16 RT tile rows = all F frames of PPW = 16 RT / F pixels per
//      wave, the first of them (sample, pixel) index gp0 = (8 tile + wave) PPW.  frame_pixel(tr, f, px) maps tile row tr = 16 i + frow
//      to its frame and its pixel among the wave's (pixel-major: gemm_tqa, frame-major: gemm_trs); global row m = (b F + f) PX + pp of
//      (sample, pixel) index gp = b PX + pp.  Rows of pixels past the tensor (gp >= npix) read as zeros.  row(i, ok, b, m, px) takes
//      what the kernel keeps per tile row.
template <int RT, int KS, class FramePixel, class Row>
VMV_DEV void rs_load_rows(u32x4_t (&a)[RT][KS], const __amdgpu_buffer_rsrc_t& a_rsrc, const int& ld, const int& gp0, const int& frow, const int& fgrp,
                                    const int F, const int& PX, const int& npix, const FramePixel& frame_pixel, const Row& row) {
#pragma unroll
    for (int i = 0; i < RT; ++i) {
        const int tr = 16 * i + frow;
        int f, px;
        frame_pixel(tr, f, px);
        const int gp = gp0 + px;
        const bool ok = gp < npix;
        const int b = gp / PX, pp = gp - b * PX;
        const long m = ((long)b * F + f) * PX + pp;
        const uint32_t avo = ok ? (uint32_t)((m * ld + 8 * fgrp) * 2) : OOB;
        row(i, ok, b, m, px);
#pragma unroll
        for (int kk = 0; kk < KS; ++kk) a[i][kk] = __builtin_amdgcn_raw_buffer_load_b128(a_rsrc, avo + (uint32_t)(kk * 64), 0, 0);
    }
}

// ---- lane swap and store path.
// v_permlane16_swap on the dword pairs (x, z) and (y, w): lanes 16-31 / 48-63 of the first dword trade places with lanes
// 0-15 / 32-47 of the second (an involution: applied twice it is the identity).  It turns the MFMA's 4-channel lane slices of two
// 16-column tiles into 8 consecutive channels of row frow per lane: columns (fgrp & 1) * 16 + (fgrp >> 1) * 8 .. + 8 of the pair.
// Inline asm with its own wait states: the builtin form compiled to `v_cvt_pk v191 / s_nop 0 / swap v188, v190 / swap v189, v191`,
// and on gfx950 the second swap then read the OLD v191 in the last four lanes of each half-wave (lanes 28-31, 60-63: output
// channels 2-3 of rows 12-15 of a tile came out as garbage, every launch) — hipcc's hazard pad for "VALU write -> v_permlane*_swap
// read" is one state short when another swap sits in between.  Four states in front cover both swaps; the operands of the
// asm statement are opaque to the scheduler, so nothing can slide in between.
VMV_DEV u32x4_t rs_swap16(u32x4_t v) {
    uint32_t x = v.x, y = v.y, z = v.z, w = v.w;
    asm("s_nop 3\n\tv_permlane16_swap_b32 %0, %2\n\tv_permlane16_swap_b32 %1, %3\n\ts_nop 1" : "+v"(x), "+v"(y), "+v"(z), "+v"(w));
    return u32x4_t{x, y, z, w};
}
// The 16-byte store of a swapped pair, always written rs_store16(rs_swap16(pair), ...): the swap is issued before the store's offset
// is worked out, as in every kernel's first form.
// Store-data discipline (cf. gemm_glds_common.h): the allocator hands the store's registers to the next row tile's
// v_pk_add_f32 at once, and with the VALU write directly behind the store the LAST dword of the last four lanes of
// every 16-lane row went out holding the new fp32 value (first GPU run of gemm_rs: every launch, rows 12-15 of a
// tile, channels 6-7 of each 8).  The data stays live — and nothing is issued — for 8 states after the store.
VMV_DEV void rs_store16(const u32x4_t o, const __amdgpu_buffer_rsrc_t out_rsrc, const uint32_t voff, const uint32_t soff) {
    __builtin_amdgcn_raw_buffer_store_b128(o, out_rsrc, voff, soff, 0);
    asm volatile("s_nop 7" ::"v"(o.x), "v"(o.y), "v"(o.z), "v"(o.w) : "memory");
}

// ---- host side
// CUs of whole XCDs (one block per CU of the persistent kernels; the column-split plan of gemm_rs).  Validation without a device
// (vmv_dry_run) neither asks the runtime nor caches the guess.
inline int rs_ncu_whole_xcds() {
    static int ncu = 0;
    if (ncu == 0) {
        int dev = 0, n = 0;
        if (vmv_dry_run || hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) n = 256;
        if (n < 8) n = 8;
        if (vmv_dry_run) return n & ~7;
        ncu = n & ~7;
    }
    return ncu;
}
// row tiles of a persistent kernel: M = B x F x P rows, a block of 8 waves holds all F frames of 8 x (rows_per_wave / F) pixels
struct RsPixelTiles { int npix, ppb, ntiles; };
inline RsPixelTiles rs_pixel_tiles(const VmvGemmParams& p, const int rows_per_wave) {
    RsPixelTiles t;
    t.npix = (int)((p.M / ((long)p.F * p.P)) * p.P);
    t.ppb = 8 * (rows_per_wave / p.F);
    t.ntiles = (t.npix + t.ppb - 1) / t.ppb;
    return t;
}

}  // namespace vmvg
