// gemm_glds_common.h — shared by the LDS-DMA GEMM kernels (gemm_glds / gemm_xglds / gemm_pglds / gemm_tfr / gemm_tqa / gemm_rs /
// gemm_ff / conv_halo): the LDS-DMA primitives and counted waits, the tile / ring configuration and fragment schedule of the
// 64-deep-chunk kernels (gemm_glds, gemm_pglds) and the store-data discipline of the staged epilogues.
#pragma once
#include "gemm_common.h"

namespace vmvg {

// Tile and ring of the 64-deep-chunk kernels: NWM x 2 waves, wave tile 16 WM x 16 WN, block tile 16 WM NWM x 32 WN, STAGES slots
// of one A + one W chunk (rows of 64 elements = 128 B).
template <int NWM, int WM, int WN, int STAGES_>
struct TileRingCfg {
    static constexpr int NW = 2 * NWM;                     // waves per block (NWM along M x 2 along N)
    static constexpr int NT = 64 * NW;
    static constexpr int STAGES = STAGES_;
    static constexpr int BM = 16 * WM * NWM;
    static constexpr int BN = 32 * WN;
    static constexpr int A_BYTES = BM * 128;
    static constexpr int W_BYTES = BN * 128;
    static constexpr int STAGE_BYTES = A_BYTES + W_BYTES;
    static constexpr int LDS_BYTES = STAGES * STAGE_BYTES;
    static constexpr int NAI = BM / (8 * NW);              // A wave-instructions per wave per chunk (8 rows each)
    static constexpr int NWI = (BN / 8 + NW - 1) / NW;     // W wave-instructions per wave per chunk
    static constexpr int LPT = NAI + NWI;                  // loads per lane per chunk
    static_assert(BM % (8 * NW) == 0, "A rows split evenly over the waves");
};
template <int WMW, int WN, int STAGES>
using GlCfg = TileRingCfg<WMW, 4, WN, STAGES>;            // gemm_glds.hip: 64-row wave tiles

// 16-byte LDS-DMA through a buffer descriptor: lane address = base + voff + soff; a lane whose voff is out of range
// (>= num_records) WRITES ZEROS to its LDS slot (verified on gfx950: tools/experiments/buffer_lds_oob.hip) — this is
// how conv zero padding and the M / N / K tails are produced without a select on 64-bit pointers.
// (the builtin is only visible to the device pass: hipcc's host pass otherwise silently drops the kernel template's
//  instantiation — stub and handle come out undefined — so the body is compiled for the device only)
VMV_DEV void blds16(__amdgpu_buffer_rsrc_t rsrc, unsigned char* lptr, uint32_t voff, uint32_t soff) {
#if defined(__HIP_DEVICE_COMPILE__)
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, (__attribute__((address_space(3))) void*)(lptr), 16, voff, soff, 0, 0);
#endif
}
// 4-byte LDS-DMA (bias / column-sum / row-statistic strips): lane l lands at lptr + 4 l, OOB lanes write zeros
VMV_DEV void blds4(__amdgpu_buffer_rsrc_t rsrc, unsigned char* lptr, uint32_t voff, uint32_t soff) {
#if defined(__HIP_DEVICE_COMPILE__)
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, (__attribute__((address_space(3))) void*)(lptr), 4, voff, soff, 0, 0);
#endif
}
constexpr uint32_t OOB = 0x80000000u;          // > num_records of every descriptor below
constexpr uint32_t SRD_RECORDS = 0x7ffffff0u;
constexpr uint32_t SRD_FLAGS = 0x00020000u;

template <int N> VMV_DEV void wait_vmcnt() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }

// run-time count (uniform): the literal must be an immediate, hence the switch
VMV_DEV void wait_vmcnt_rt(int n) {
    switch (n) {
        case 0: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;
        case 1: asm volatile("s_waitcnt vmcnt(1)" ::: "memory"); break;
        case 2: asm volatile("s_waitcnt vmcnt(2)" ::: "memory"); break;
        case 3: asm volatile("s_waitcnt vmcnt(3)" ::: "memory"); break;
        case 4: asm volatile("s_waitcnt vmcnt(4)" ::: "memory"); break;
        case 5: asm volatile("s_waitcnt vmcnt(5)" ::: "memory"); break;
        case 6: asm volatile("s_waitcnt vmcnt(6)" ::: "memory"); break;
        case 7: asm volatile("s_waitcnt vmcnt(7)" ::: "memory"); break;
        case 8: asm volatile("s_waitcnt vmcnt(8)" ::: "memory"); break;
        case 9: asm volatile("s_waitcnt vmcnt(9)" ::: "memory"); break;
        case 10: asm volatile("s_waitcnt vmcnt(10)" ::: "memory"); break;
        case 11: asm volatile("s_waitcnt vmcnt(11)" ::: "memory"); break;
        case 12: asm volatile("s_waitcnt vmcnt(12)" ::: "memory"); break;
        case 13: asm volatile("s_waitcnt vmcnt(13)" ::: "memory"); break;
        case 14: asm volatile("s_waitcnt vmcnt(14)" ::: "memory"); break;
        case 15: asm volatile("s_waitcnt vmcnt(15)" ::: "memory"); break;
        case 16: asm volatile("s_waitcnt vmcnt(16)" ::: "memory"); break;
        case 17: asm volatile("s_waitcnt vmcnt(17)" ::: "memory"); break;
        case 18: asm volatile("s_waitcnt vmcnt(18)" ::: "memory"); break;
        case 19: asm volatile("s_waitcnt vmcnt(19)" ::: "memory"); break;
        case 20: asm volatile("s_waitcnt vmcnt(20)" ::: "memory"); break;
        case 21: asm volatile("s_waitcnt vmcnt(21)" ::: "memory"); break;
        case 22: asm volatile("s_waitcnt vmcnt(22)" ::: "memory"); break;
        case 23: asm volatile("s_waitcnt vmcnt(23)" ::: "memory"); break;
        case 24: asm volatile("s_waitcnt vmcnt(24)" ::: "memory"); break;
        default: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;
    }
}

// ---- fragment schedule of the 64-deep-chunk kernels.  Lane (frow = lane & 15, fgrp = lane >> 4) reads k-slice kk * 4 + fgrp of row
//      frow of every 16-row fragment of its wave tile; the row keeps logical 16-B slot s at s ^ fswz, fswz = (frow >> 1) & 7 (the loaders).
template <class Cfg, int WM, int WN>
VMV_DEV void read_frags(const unsigned char* smem, int slot_idx, int kk, int wave_m, int wave_n, int frow, int fgrp, int fswz, elem8_t (&af)[WM],
                        elem8_t (&wf)[WN]) {
    const u32x4_t* a = reinterpret_cast<const u32x4_t*>(smem + slot_idx * Cfg::STAGE_BYTES) + (wave_m * 16 * WM + frow) * 8;
    const u32x4_t* w = reinterpret_cast<const u32x4_t*>(smem + slot_idx * Cfg::STAGE_BYTES + Cfg::A_BYTES) +
                       (wave_n * 16 * WN + frow) * 8;
    const int slot = (kk * 4 + fgrp) ^ fswz;
#pragma unroll
    for (int i = 0; i < WM; ++i) af[i] = __builtin_bit_cast(elem8_t, a[i * 16 * 8 + slot]);
#pragma unroll
    for (int j = 0; j < WN; ++j) wf[j] = __builtin_bit_cast(elem8_t, w[j * 16 * 8 + slot]);
}
template <int WM, int WN>
VMV_DEV void mma_tile(f32x4_t (&acc)[WN][WM], const elem8_t (&af)[WM], const elem8_t (&wf)[WN]) {
#pragma unroll
    for (int j = 0; j < WN; ++j)
#pragma unroll
        for (int i = 0; i < WM; ++i)
            acc[j][i] = VMV_MFMA16(wf[j], af[i], acc[j][i], 0, 0, 0);
}

// ---- store-data discipline of the staged epilogues.  A loop of the form "read unit r from LDS -> store it -> read unit r + 1 into the
//      same registers" compiles to `buffer_store_dwordx4 v[a:a+3]` directly followed by `ds_read_b128 v[a:a+3]`, and on gfx950 an LDS
//      read that RETURNS into a pending store's data registers corrupts the store when the store path is backed up (seen as wrong / zero
//      column pairs in some 16-lane groups; found with the retired wave-specialised kernel, whose 168 registers made the allocator reuse
//      registers at once).  So store data is always a VALU-written copy — valu_copy() — never an LDS-read destination, and the previous
//      copy is kept alive — keep_alive(), after the wait for the LDS reads — until the next LDS reads have returned.
VMV_DEV u32x4_t valu_copy(const u32x4_t v) {
    u32x4_t sd;
    asm volatile("v_mov_b32 %0, %4\n\tv_mov_b32 %1, %5\n\tv_mov_b32 %2, %6\n\tv_mov_b32 %3, %7"
                 : "=&v"(sd.x), "=&v"(sd.y), "=&v"(sd.z), "=&v"(sd.w)
                 : "v"(v.x), "v"(v.y), "v"(v.z), "v"(v.w));
    return sd;
}
VMV_DEV void keep_alive(const u32x4_t& v) { asm volatile("" ::"v"(v)); }

}  // namespace vmvg
