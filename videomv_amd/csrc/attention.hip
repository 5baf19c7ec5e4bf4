// attention.hip — softmax(Q K^T * scale) V on gfx950 for head_dim 32, 64 and 128; operands and output in the 16-bit element type of
// the build (fp16 or bf16: common.h), fp32 softmax + accumulate.  Index maps (include/vmv.h) serve the UNet's three attention shapes —
// spatial self (N = H*W), spatial cross (Nk = 77 text tokens), per-pixel temporal (N = 24 frames) — the LGM U-Net and the CLIP towers.
// Three kernels on shared device parts; attn_decide() picks one and vmv_attention launches it from one table:
//   attn_block_kernel<QT, D, CAUSAL>  four waves share one (problem, head, tile of 64 QT queries) and one K / V ring in LDS, filled by
//                                     LDS-DMA: head_dim 64 with 128- or 256-query blocks or causal, head_dim 32 and 128;
//   attn_wave_kernel                  one wave per problem (Nq <= 32 < Nk, head_dim 64), 64-key tiles, a private V^T stage, no barrier;
//   attn_short_kernel                 one wave per problem (Nq, Nk <= 32, head_dim 64), every load issued before the first use.
//
// Formulation (everything transposed so that softmax statistics are lane-local):
//   S^T = K Q^T  : MFMA A = K fragment (rows = keys), B = Q fragment (cols = queries)
//                  -> lane (u = lane&15, g = lane>>4) holds S[q = u][4 keys] per 16-key tile
//   O^T = V^T P^T: MFMA A = V^T fragment (rows = d),  B = P^T fragment (cols = queries)
//                  -> lane holds O[q = u][d = 16*dt + 4*g + r]: the same q as its softmax state, so the
//                     running max / sum / rescale never cross lanes, and the output store is 8 bytes per lane.
// The K rows of each 16-key MFMA tile are loaded in a permuted order (tile t, row u -> key 32*(t>>1) + 8*(u>>2)
// + 4*(t&1) + (u&3)) so that the exponentiated S^T registers of tiles (2kk, 2kk+1) ARE the P^T B-operand for
// keys 32kk + 8g + 0..7 — no shuffles and no LDS round trip between the two GEMMs.
// Online softmax of the 64-key tile loops (block and wave kernels; per lane: query u, 16 keys of the tile).  The softmax VALU work,
// not the 32 MFMAs, bounds a tile (16 quarter-rate v_exp per query tile alone cost as much as the tile's MFMAs), so it is kept
// minimal: the running max is tracked on the RAW scores (scale > 0) and the scale is folded into one FMA per score,
// exp2((s - m) * sc) = exp2(fma(s, sc, -m * sc)); key masking runs only on a partial last tile; the accumulator rescale is
// skipped while no lane of the wave sees a new maximum.
#include "common.h"
#include "gemm_glds_common.h"       // LDS-DMA helper, buffer descriptor constants

namespace {

VMV_DEV long seq_base(const VmvSeqMap& m, int o) {
    return (long)(o / m.inner) * m.s_outer + (long)(o % m.inner) * m.s_inner;
}
VMV_DEV int k_swz(int key) { return (((key >> 3) & 3) << 1) | ((key >> 1) & 1); }

constexpr float NEG_BIG = -1.0e30f;

// ---------------------------------------------------------------------------------------------- parts shared by the kernels
// (straight-line parts only: a part with a branch or a loop nest of its own is simplified before it is inlined, and the kernels then
//  come out with other instructions and more registers — profiles/attn_family_kernel_resources.txt lists the forms that did)
// The four operand base pointers of problem o, head h (D = head dimension)
struct AttnBase { const uint16_t *q, *k, *v; uint16_t* o; };
VMV_DEV AttnBase attn_base(const VmvAttnParams& p, const int o, const int h, const int D) {
    return {reinterpret_cast<const uint16_t*>(p.q) + seq_base(p.qm, o) + h * D,
            reinterpret_cast<const uint16_t*>(p.k) + seq_base(p.km, o / p.kv_div) + h * D,
            reinterpret_cast<const uint16_t*>(p.v) + seq_base(p.vm, o / p.kv_div) + h * D,
            reinterpret_cast<uint16_t*>(p.o) + seq_base(p.om, o) + h * D};
}
// (o, h) are wave-uniform (block indices, or blockIdx * 4 + wave), so the four problem base pointers are too — but not
// provably so for the compiler (threadIdx >> 6), which kept them in 8 VGPRs and spilled four of them across the main loop of
// the 256-query block kernel.  Through readfirstlane they live in SGPRs and every access becomes scalar base + 32-bit lane offset.
template <typename T> VMV_DEV T* uniform_ptr(T* ptr) {
    const uint64_t a = reinterpret_cast<uint64_t>(ptr);
    // (the builtin returns a signed int: widen through uint32_t, or a low word with bit 31 set smears into the high half)
    const uint64_t u = ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)(a >> 32)) << 32) |
                       (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)a);
    return reinterpret_cast<T*>(u);
}
VMV_DEV AttnBase uniform_base(const AttnBase& b) { return {uniform_ptr(b.q), uniform_ptr(b.k), uniform_ptr(b.v), uniform_ptr(b.o)}; }

// 16 bytes of an operand row, zeros for a row outside the problem; load_frag: as an MFMA fragment (Q: the B operand, row q at
// k-slot kk * 32 + 8 * g; K read straight from global memory: the A operand, likewise)
VMV_DEV u32x4_t load16(const uint16_t* ptr, const bool valid) {
    u32x4_t v = {0u, 0u, 0u, 0u};
    if (valid) v = *reinterpret_cast<const u32x4_t*>(ptr);
    return v;
}
VMV_DEV elem8_t load_frag(const uint16_t* ptr, const bool valid) { return __builtin_bit_cast(elem8_t, load16(ptr, valid)); }

// Maximum of a query's scores in the lane's NT tiles and in lane ^ 16's.
// (v_max3 through asm: fmaxf() is llvm.maxnum, which in IEEE mode first quiets every MFMA result with a v_max x, x — 12 extra
//  instructions per query tile; the cross-lane steps are gfx950's VALU lane swaps instead of two ds_bpermute round trips)
template <int NT> VMV_DEV float score_max(const f32x4_t (&s)[NT]) {
    float mx = vmax3(s[0][0], s[0][1], s[0][2]);
#pragma unroll
    for (int i = 3; i < 4 * NT - 1; i += 2) mx = vmax3(mx, s[i >> 2][i & 3], s[(i + 1) >> 2][(i + 1) & 3]);
    mx = vmax2(mx, s[NT - 1][3]);
    return xor16_max(mx);
}

// pv = P = exp2(s * sc + nm) of the lane's NT score tiles (packed fp32: one v_pk_fma / v_pk_add per two scores); returns the two
// halves of their sum.  pack_pt: the exponentiated tiles (2 kk, 2 kk + 1) as the P^T B operand for keys 32 kk + 8 g + 0..7.
template <int NT> VMV_DEV f32x2_t exp_scores(const f32x4_t (&s)[NT], float (&pv)[NT][4], const float sc, const float nm) {
    const f32x2_t sc2 = {sc, sc}, nm2 = {nm, nm};
    f32x2_t ps2 = {0.f, 0.f};
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        f32x2_t a = {s[t][0], s[t][1]}, b = {s[t][2], s[t][3]};
        a = a * sc2 + nm2; b = b * sc2 + nm2;
        const f32x2_t ea = {__builtin_amdgcn_exp2f(a.x), __builtin_amdgcn_exp2f(a.y)};
        const f32x2_t eb = {__builtin_amdgcn_exp2f(b.x), __builtin_amdgcn_exp2f(b.y)};
        pv[t][0] = ea.x; pv[t][1] = ea.y; pv[t][2] = eb.x; pv[t][3] = eb.y;
        ps2 += ea; ps2 += eb;
    }
    return ps2;
}
VMV_DEV elem8_t pack_pt(const float (&lo)[4], const float (&hi)[4]) {
    u32x4_t w;
    w.x = pack_elem2(lo[0], lo[1]); w.y = pack_elem2(lo[2], lo[3]);
    w.z = pack_elem2(hi[0], hi[1]); w.w = pack_elem2(hi[2], hi[3]);
    return __builtin_bit_cast(elem8_t, w);
}

// The private V^T stage of a wave (wave and short kernels): [64 d][KEYS keys], element (d, key) at Vt[d * KEYS + (key ^ 8 * swz(d))],
// swz(d) = ((d >> 3) ^ (d >> 1)) & (KEYS / 8 - 1), so that the eight 2-byte writes of a piece and the 16-byte fragment reads are
// both bank-conflict free.  vt_write puts the 16-byte piece (key, d = 8 * slot + 0..7) there, vt_frag reads the A operand of row d
// for keys 8 * kblock + 0..7.  The stage is the wave's own: no block barrier, a wave's LDS instructions execute in order.
template <int KEYS> VMV_DEV void vt_write(uint16_t* Vt, const int key, const int slot, const u32x4_t& vv) {
    const uint32_t w[4] = {vv.x, vv.y, vv.z, vv.w};
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int d = slot * 8 + j;
        const int fk = ((slot ^ ((slot << 2) | (j >> 1))) & (KEYS / 8 - 1)) << 3;    // = 8 * swz(d): d >> 3 = slot, d >> 1 = 4 * slot + (j >> 1)
        Vt[d * KEYS + (key ^ fk)] = (j & 1) ? (uint16_t)(w[j >> 1] >> 16) : (uint16_t)(w[j >> 1] & 0xffffu);
    }
}
template <int KEYS> VMV_DEV elem8_t vt_frag(const uint16_t* Vt, const int d, const int kblock) {
    const int fsl = ((d >> 3) ^ (d >> 1)) & (KEYS / 8 - 1);
    return __builtin_bit_cast(elem8_t, reinterpret_cast<const u32x4_t*>(Vt)[d * (KEYS / 8) + (kblock ^ fsl)]);
}

// Normalise and store one query row's part of the output: the lane owns O[q][d = 16 dt + 4 g + 0..3], orow = &O[q][4 g]
template <int DT> VMV_DEV void store_o(uint16_t* orow, const f32x4_t (&oacc)[DT], const float inv) {
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) {
        const f32x4_t a = oacc[dt] * inv;
        u32x2_t w;
        w.x = pack_elem2(a.x, a.y); w.y = pack_elem2(a.z, a.w);
        *reinterpret_cast<u32x2_t*>(orow + dt * 16) = w;
    }
}

constexpr int attn_kbytes(int D) { return D == 128 ? 16384 : 8192; }           // a staged K tile, and a staged V tile, of the block kernel
constexpr int attn_block_lds(int D) { return 2 * 2 * attn_kbytes(D); }          // its ring: two stages of K | V

// ------------------------------------------------------------------------------------------------------------- block kernel
// Four waves share one (problem, head, tile of 64 QT queries) and one K / V ring.
// QT = 16-query tiles per wave (QT = 4: 64 queries per wave, 256 per block — every K / V fragment read from LDS and
// every staged K / V tile then serves twice the MFMAs; the LDS port, shared by all the blocks of a CU, is what bounds the
// 128-query version at long sequences)
// D = head dimension: 64 (the video UNet), 32 (the LGM U-Net's 512-channel / 16-head MVAttention) or 128 (the CLIP image tower's
// zero-padded heads): D / 32 k-steps in S^T = K Q^T, D / 16 output tiles in O^T = V^T P^T and D / 8 16-byte slots per staged K row.
// CAUSAL: keys j > query i masked out (own instantiation: the test costs <4, 64> two spilled registers)
template <int QT, int D = 64, bool CAUSAL = false>
__global__ __launch_bounds__(256, 2) void attn_block_kernel(const VmvAttnParams p, const int /* problems: the per-wave kernels' */) {
    VMV_KERNEL_ENTER();
    static_assert(D == 32 || D == 64 || D == 128, "head_dim 32, 64 or 128");
    constexpr int KK = D / 32, DT = D / 16, SLOTS = D / 8, SLOG = (D == 128) ? 4 : (D == 64) ? 3 : 2;
    constexpr int KBYTES = attn_kbytes(D), STAGE = 2 * KBYTES;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const int tid = threadIdx.x, lane = tid & 63, u = lane & 15, g = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);

    // ---- which problem / query rows does this wave own?
    // XCD-aware block map: workgroups are handed out round-robin over the 8 XCDs in linear block order, so with the natural map
    // the query tiles that share one (problem, head)'s K / V land on eight different L2s and each re-fetches them from the fabric
    // (FETCH_SIZE: 1.2 GB per L0 self-attention launch for 236 MB of operands).  Bijection: the blocks of one XCD, in issue
    // order, walk consecutive logical ids = the query tiles of one (problem, head), then the next pair.
    const int nqt = gridDim.x, nh = gridDim.y;
    const int lin = blockIdx.x + nqt * (blockIdx.y + nh * blockIdx.z), nblk = nqt * nh * gridDim.z;
    const int qq = nblk >> 3, rr = nblk & 7, xcd = lin & 7, idx = lin >> 3;
    const int logical = (xcd < rr ? xcd * (qq + 1) : rr * (qq + 1) + (xcd - rr) * qq) + idx;
    const int pair = logical / nqt, qtile = logical - pair * nqt;
    const int o = pair / nh, h = pair - o * nh, q0 = (qtile * 4 + wave) * (16 * QT);
    const AttnBase b = uniform_base(attn_base(p, o, h, D));
    // row offsets inside one problem fit 32 bits (vmv_attention checks (N - 1) * s_row + head_dim < 2^30 elements): 64-bit
    // products of the row index kept their sign-extension registers alive across the main loop (three more spilled pairs)
    const int qs_row = (int)p.qm.s_row, ks_row = (int)p.km.s_row, vs_row = (int)p.vm.s_row, os_row = (int)p.om.s_row;

    // ---- Q fragments (B operand): row q0 + 16*qt + u, k-slot kk*32 + 8*g
    elem8_t qf[QT][KK];
#pragma unroll
    for (int qt = 0; qt < QT; ++qt) {
        const int q = q0 + qt * 16 + u;
#pragma unroll
        for (int kk = 0; kk < KK; ++kk) qf[qt][kk] = load_frag(b.q + q * qs_row + kk * 32 + g * 8, q < p.Nq);
    }

    f32x4_t oacc[QT][DT];
    float m_run[QT], l_run[QT];
#pragma unroll
    for (int qt = 0; qt < QT; ++qt) {
        m_run[qt] = NEG_BIG; l_run[qt] = 0.f;
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) oacc[qt][dt] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    }
    const float sc = p.scale * 1.44269504088896341f;   // exp2 domain (> 0)

    const int ntile = (p.Nk + 63) >> 6;
    // K / V ring: two LDS stages, each the K tile ([64 keys][SLOTS] 16-byte pieces, XOR-swizzled) then the V tile (the image of the
    // transpose read below).  The next tile's loads are issued BEFORE the current tile's MFMAs into the other stage (one barrier
    // per tile, HBM/L2 latency hidden under the math), and go global -> LDS by DMA (was global -> registers -> ds_write, 21 % of the
    // kernel by ablation): a wave-instruction fills 1 KB of the stage lane-linearly, so the lane FETCHES the piece whose place it
    // writes — both images are permutations of 16-byte pieces.  Rows >= Nk fall outside the descriptors and arrive as zeros
    // (0 x NaN from a recycled buffer would poison P.V).
    constexpr int NPIECE = (64 * SLOTS) / 256;      // 16-byte pieces of K (and of V) per lane per tile
    uint32_t k_off[NPIECE], v_off[NPIECE];
    unsigned char* ring = smem_raw;                 // (a plain variable: const, or smem_raw itself in issue_tile, costs <2, 64> four registers)
    const __amdgpu_buffer_rsrc_t k_rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint16_t*>(b.k), 0, (uint32_t)((p.Nk - 1) * ks_row + D) * 2u, vmvg::SRD_FLAGS);
    const __amdgpu_buffer_rsrc_t v_rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint16_t*>(b.v), 0, (uint32_t)((p.Nk - 1) * vs_row + D) * 2u, vmvg::SRD_FLAGS);
#pragma unroll
    for (int i = 0; i < NPIECE; ++i) {
        const int q = (wave * NPIECE + i) * 64 + lane;                   // piece of the tile image this lane fills
        const int krow = q >> SLOG, ksl = (q & (SLOTS - 1)) ^ (k_swz(krow) & (SLOTS - 1));
        k_off[i] = (uint32_t)(krow * ks_row + ksl * 8) * 2u;
        const int dt = q >> 7, r = q & 127;                              // V image: 2 KB (128 pieces) per 16-d subtile
        const int pos = (r >> 3) ^ (dt & 1);
        const int vrow = (((pos >> 3) & 1) << 5) | ((pos & 3) << 3) | (((pos >> 2) & 1) << 2) | ((r >> 1) & 3);
        v_off[i] = (uint32_t)(vrow * vs_row + (dt * 2 + (r & 1)) * 8) * 2u;
    }
    auto issue_tile = [&](int kt2, int buf) {
        unsigned char* kd = ring + buf * STAGE + wave * (NPIECE * 1024);
        const uint32_t kb = (uint32_t)(kt2 * 64 * ks_row) * 2u, vb = (uint32_t)(kt2 * 64 * vs_row) * 2u;
#pragma unroll
        for (int i = 0; i < NPIECE; ++i) {
            vmvg::blds16(k_rsrc, kd + i * 1024, k_off[i] + kb, 0);
            vmvg::blds16(v_rsrc, kd + KBYTES + i * 1024, v_off[i] + vb, 0);
        }
    };
    // V stays ROW-major in LDS — one 16-byte piece per (key, 8 d) instead of eight scattered 2-byte writes of a
    // transposed image — and the PV fragments come from gfx950's transpose read: ds_read_b64_tr_b16 hands lane j of a
    // 16-lane group column j of the [4 rows][16 columns] block whose row j / 4, columns 4 (j % 4)..+3 the lanes address
    // (tools/experiments/tr_probe.hip).  Image: per 16-d subtile (2 KB) sixteen 128-byte blocks of [4 keys][16 d]; the
    // block of keys 32 kk + 8 g + 4 h + 0..3 sits at position (8 kk + 4 h + g) ^ (dt & 1), so that the two lane groups
    // of a half-wave (g, g + 1) read different 128-byte bank halves: piece (key, slot) at dt * 2048 + (pos << 7) + ((key & 3) << 5)
    // + ((slot & 1) << 4), dt = slot >> 1, pos = (((key >> 5) << 3) + (((key >> 2) & 1) << 2) + ((key >> 3) & 3)) ^ (dt & 1)
    // (issue_tile above inverts this).  K image: [key][slot ^ swizzle(key)].
    issue_tile(0, 0);
    vmvg::wait_vmcnt<0>();
    __syncthreads();
    for (int kt = 0; kt < ntile; ++kt) {
        const int key0 = kt * 64;
        if (kt + 1 < ntile) issue_tile(kt + 1, (kt + 1) & 1);      // the other stage: last read one tile ago, behind a barrier
        const u32x4_t* Ks = reinterpret_cast<const u32x4_t*>(ring + (kt & 1) * STAGE);
        const unsigned char* Vs = ring + (kt & 1) * STAGE + KBYTES;

        // ---- S^T tiles (two query tiles at a time: the K fragments stay in registers for all QT of them) + online softmax
        elem8_t kf[4][KK];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int krow = 32 * (t >> 1) + 8 * (u >> 2) + 4 * (t & 1) + (u & 3);
            const int ksw = k_swz(krow);
#pragma unroll
            for (int kk = 0; kk < KK; ++kk) kf[t][kk] = __builtin_bit_cast(elem8_t, Ks[krow * SLOTS + ((kk * 4 + g) ^ (ksw & (SLOTS - 1)))]);
        }
        elem8_t pf[QT][2];
        const bool partial = key0 + 64 > p.Nk;                 // uniform
#pragma unroll
        for (int qp = 0; qp < QT / 2; ++qp) {
            f32x4_t s[2][4];
#pragma unroll
            for (int q2 = 0; q2 < 2; ++q2)
#pragma unroll
                for (int t = 0; t < 4; ++t) s[q2][t] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int kk = 0; kk < KK; ++kk)
#pragma unroll
                    for (int q2 = 0; q2 < 2; ++q2)
                        s[q2][t] = VMV_MFMA16(kf[t][kk], qf[2 * qp + q2][kk], s[q2][t], 0, 0, 0);
#pragma unroll
            for (int q2 = 0; q2 < 2; ++q2) {
                const int qt = 2 * qp + q2;
                if (partial || CAUSAL) {         // (causal: key <= query — the CLIP text tower; key 0 is visible to every query, so the
                                                 //  running max is real from the first tile on and masked scores exponentiate to 0)
                    const int qlim = CAUSAL ? q0 + qt * 16 + u : 0x7fffffff;
#pragma unroll
                    for (int t = 0; t < 4; ++t) {
                        const int kb = key0 + 32 * (t >> 1) + 8 * g + 4 * (t & 1);
#pragma unroll
                        for (int r = 0; r < 4; ++r)
                            if (kb + r >= p.Nk || kb + r > qlim) s[q2][t][r] = NEG_BIG;
                    }
                }
                const float m_old = m_run[qt];
                const float m_new = xor32_max3(score_max<4>(s[q2]), m_old);
                float pv[4][4];
                const f32x2_t ps2 = exp_scores<4>(s[q2], pv, sc, -m_new * sc);
                const float psum = ps2.x + ps2.y;
                if (__builtin_amdgcn_ballot_w64(m_new != m_old) != 0ull) {          // some query of this wave has a new maximum
                    const float alpha = __builtin_amdgcn_exp2f((m_old - m_new) * sc);
                    m_run[qt] = m_new;
                    l_run[qt] *= alpha;
#pragma unroll
                    for (int dt = 0; dt < DT; ++dt) oacc[qt][dt] *= alpha;
                }
                l_run[qt] += psum;
#pragma unroll
                for (int kk = 0; kk < 2; ++kk) pf[qt][kk] = pack_pt(pv[2 * kk], pv[2 * kk + 1]);
            }
        }
        // ---- O^T += V^T P^T
        const unsigned char* vlane = Vs + ((u >> 2) << 5) + ((u & 3) << 3);
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) {
#pragma unroll
            for (int kk = 0; kk < 2; ++kk) {
#if defined(__HIP_DEVICE_COMPILE__)
                typedef short s16x4_t __attribute__((ext_vector_type(4)));
                typedef __attribute__((address_space(3))) s16x4_t* lds_s16x4_p;
                const unsigned char* b0 = vlane + dt * 2048 + (((kk * 8 + g) ^ (dt & 1)) << 7);
                const unsigned char* b1 = vlane + dt * 2048 + (((kk * 8 + 4 + g) ^ (dt & 1)) << 7);
                const s16x4_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_p)(b0));
                const s16x4_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_p)(b1));
                const u32x2_t lo2 = __builtin_bit_cast(u32x2_t, lo), hi2 = __builtin_bit_cast(u32x2_t, hi);
                const elem8_t vf = __builtin_bit_cast(elem8_t, u32x4_t{lo2.x, lo2.y, hi2.x, hi2.y});
#else
                const elem8_t vf = {};
                (void)vlane;
#endif
#pragma unroll
                for (int qt = 0; qt < QT; ++qt) oacc[qt][dt] = VMV_MFMA16(vf, pf[qt][kk], oacc[qt][dt], 0, 0, 0);
            }
        }
        vmvg::wait_vmcnt<0>();                             // my pieces of tile kt + 1 have landed ...
        __syncthreads();                                   // ... and everyone's; everyone is done reading tile kt
    }
    // ---- normalise and store: lane owns O[q = q0 + 16 qt + u][d = 16 dt + 4 g + 0..3]
#pragma unroll
    for (int qt = 0; qt < QT; ++qt) {
        const float l = xor16_32_sum(l_run[qt]);
        const float inv = 1.0f / l;
        const int q = q0 + qt * 16 + u;
        if (q < p.Nq) store_o<DT>(b.o + q * os_row + 4 * g, oacc[qt], inv);
    }
}

// -------------------------------------------------------------------------------------------------------------- wave kernel
// One problem per wave (Nq <= 32 < Nk, head_dim 64: the cross-attention of the smallest levels — HBM-bound), 64-key tiles.  Only V^T
// goes through LDS — the K fragments are 16 contiguous bytes of a key row and are loaded straight into registers — so a wave
// needs 8 KB instead of 16 (5 blocks per CU instead of 2), and the stage is private: no block barriers.
__global__ __launch_bounds__(256, 2) void attn_wave_kernel(const VmvAttnParams p, const int nproblems) {
    VMV_KERNEL_ENTER();
    constexpr int QT = 2, KK = 2, DT = 4;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, u = lane & 15, g = lane >> 4;
    const int pidx = blockIdx.x * 4 + wave;
    const bool wvalid = pidx < nproblems;              // an idle wave of the last block walks problem 0 with every access masked
    const int pi = wvalid ? pidx : 0;
    const AttnBase b = uniform_base(attn_base(p, pi / p.heads, pi % p.heads, 64));
    const int qs_row = (int)p.qm.s_row, ks_row = (int)p.km.s_row, vs_row = (int)p.vm.s_row, os_row = (int)p.om.s_row;   // (as the block kernel)
    uint16_t* Vt = reinterpret_cast<uint16_t*>(smem_raw + wave * 8192);

    elem8_t qf[QT][KK];
#pragma unroll
    for (int qt = 0; qt < QT; ++qt) {
        const int q = qt * 16 + u;
#pragma unroll
        for (int kk = 0; kk < KK; ++kk) qf[qt][kk] = load_frag(b.q + q * qs_row + kk * 32 + g * 8, wvalid && q < p.Nq);
    }

    f32x4_t oacc[QT][DT];
    float m_run[QT], l_run[QT];
#pragma unroll
    for (int qt = 0; qt < QT; ++qt) {
        m_run[qt] = NEG_BIG; l_run[qt] = 0.f;
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) oacc[qt][dt] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    }
    const float sc = p.scale * 1.44269504088896341f;   // exp2 domain (> 0)

    const int ntile = (p.Nk + 63) >> 6;
    for (int kt = 0; kt < ntile; ++kt) {
        const int key0 = kt * 64;
        __builtin_amdgcn_s_waitcnt(0xc07f);   // previous tile's fragment reads are done
        asm volatile("" ::: "memory");
        u32x4_t vvr[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int idx = lane + i * 64;
            const int key = key0 + (idx >> 3);
            vvr[i] = load16(b.v + key * vs_row + (idx & 7) * 8, wvalid && key < p.Nk);
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) vt_write<64>(Vt, (lane + i * 64) >> 3, (lane + i * 64) & 7, vvr[i]);
        __builtin_amdgcn_s_waitcnt(0xc07f);
        asm volatile("" ::: "memory");

        // ---- S^T tiles + online softmax (as the block kernel, for its two query tiles)
        elem8_t kf[4][KK];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int key = key0 + 32 * (t >> 1) + 8 * (u >> 2) + 4 * (t & 1) + (u & 3);
#pragma unroll
            for (int kk = 0; kk < KK; ++kk) kf[t][kk] = load_frag(b.k + key * ks_row + kk * 32 + g * 8, wvalid && key < p.Nk);
        }
        elem8_t pf[QT][2];
        const bool partial = key0 + 64 > p.Nk;                 // uniform
        f32x4_t s[QT][4];
#pragma unroll
        for (int qt = 0; qt < QT; ++qt)
#pragma unroll
            for (int t = 0; t < 4; ++t) s[qt][t] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int kk = 0; kk < KK; ++kk)
#pragma unroll
                for (int qt = 0; qt < QT; ++qt)
                    s[qt][t] = VMV_MFMA16(kf[t][kk], qf[qt][kk], s[qt][t], 0, 0, 0);
#pragma unroll
        for (int qt = 0; qt < QT; ++qt) {
            if (partial) {
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const int kb = key0 + 32 * (t >> 1) + 8 * g + 4 * (t & 1);
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        if (kb + r >= p.Nk) s[qt][t][r] = NEG_BIG;
                }
            }
            const float m_old = m_run[qt];
            const float m_new = xor32_max3(score_max<4>(s[qt]), m_old);
            float pv[4][4];
            const f32x2_t ps2 = exp_scores<4>(s[qt], pv, sc, -m_new * sc);
            const float psum = ps2.x + ps2.y;
            if (__builtin_amdgcn_ballot_w64(m_new != m_old) != 0ull) {          // some query of this wave has a new maximum
                const float alpha = __builtin_amdgcn_exp2f((m_old - m_new) * sc);
                m_run[qt] = m_new;
                l_run[qt] *= alpha;
#pragma unroll
                for (int dt = 0; dt < DT; ++dt) oacc[qt][dt] *= alpha;
            }
            l_run[qt] += psum;
#pragma unroll
            for (int kk = 0; kk < 2; ++kk) pf[qt][kk] = pack_pt(pv[2 * kk], pv[2 * kk + 1]);
        }
        // ---- O^T += V^T P^T
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) {
#pragma unroll
            for (int kk = 0; kk < 2; ++kk) {
                const elem8_t vf = vt_frag<64>(Vt, dt * 16 + u, kk * 4 + g);
#pragma unroll
                for (int qt = 0; qt < QT; ++qt) oacc[qt][dt] = VMV_MFMA16(vf, pf[qt][kk], oacc[qt][dt], 0, 0, 0);
            }
        }
    }
#pragma unroll
    for (int qt = 0; qt < QT; ++qt) {
        const float l = xor16_32_sum(l_run[qt]);
        const float inv = 1.0f / l;
        const int q = qt * 16 + u;
        if (wvalid && q < p.Nq) store_o<DT>(b.o + q * os_row + 4 * g, oacc[qt], inv);
    }
}

// ------------------------------------------------------------------------------------------------------------- short kernel
// Short problems (Nq, Nk <= 32: the 24-frame temporal attention of every pixel x head) — HBM-bound.
// One wave per problem, as attn_wave_kernel, but built for memory-level parallelism instead of generality:
//   * every global load of the problem (Q: 2, K: 4, V: 4 wave-instructions of 16 B per lane) is issued before the first
//     use, so a wave pays ONE memory round trip instead of three dependent ones;
//   * only the 32-key half that can hold valid keys exists: 2 S^T tiles instead of 4, one P.V k-step instead of 2 (half
//     the MFMAs, the exponentials and the registers: 4-5 waves per SIMD instead of 2-3), and the V^T stage is
//     [64 d][32 keys] = 4 KB per wave, filled from the 4 valid row groups only (32 instead of 64 16-bit LDS writes).
__global__ __launch_bounds__(256, 4) void attn_short_kernel(const VmvAttnParams p, const int nproblems) {
    VMV_KERNEL_ENTER();
    __shared__ __attribute__((aligned(16))) unsigned char smem_s[4 * 4096];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, u = lane & 15, g = lane >> 4;
    const int pidx = blockIdx.x * 4 + wave;
    if (pidx >= nproblems) return;                      // (no block-level synchronisation below)
    const AttnBase b = attn_base(p, pidx / p.heads, pidx % p.heads, 64);
    uint16_t* Vt = reinterpret_cast<uint16_t*>(smem_s + wave * 4096);

    // ---- all loads of the problem, back to back
    elem8_t qf[2][2], kf[2][2];
    u32x4_t vv[4];
#pragma unroll
    for (int qt = 0; qt < 2; ++qt) {
        const int q = qt * 16 + u;
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) qf[qt][kk] = load_frag(b.q + (long)q * p.qm.s_row + kk * 32 + g * 8, q < p.Nq);
    }
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const int key = 8 * (u >> 2) + 4 * t + (u & 3);          // permuted key order (file header), keys 0..31
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) kf[t][kk] = load_frag(b.k + (long)key * p.km.s_row + kk * 32 + g * 8, key < p.Nk);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int key = (lane >> 3) + 8 * i;
        vv[i] = load16(b.v + (long)key * p.vm.s_row + (lane & 7) * 8, key < p.Nk);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) vt_write<32>(Vt, (lane >> 3) + 8 * i, lane & 7, vv[i]);
    // ---- S^T = K Q^T (2 key tiles x 2 query tiles) and the softmax of each query over its <= 32 keys
    const float sc = p.scale * 1.44269504088896341f;
    elem8_t pf[2];
    float linv[2];
#pragma unroll
    for (int qt = 0; qt < 2; ++qt) {
        f32x4_t s[2];
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            s[t] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int kk = 0; kk < 2; ++kk) s[t] = VMV_MFMA16(kf[t][kk], qf[qt][kk], s[t], 0, 0, 0);
        }
        // lane (u, g) holds the scores of query 16 qt + u against keys 8 g + 4 t + r
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (8 * g + 4 * t + r >= p.Nk) s[t][r] = NEG_BIG;
        const float mx = xor32_max3(score_max<2>(s), NEG_BIG);
        float e[2][4], psum = 0.f;
        exp_scores<2>(s, e, sc, -mx * sc);
#pragma unroll
        for (int t = 0; t < 2; ++t)                     // (summed in key order, not from the packed halves exp_scores returns)
#pragma unroll
            for (int r = 0; r < 4; ++r) psum += e[t][r];
        linv[qt] = 1.0f / xor16_32_sum(psum);
        pf[qt] = pack_pt(e[0], e[1]);                   // = P^T B-operand for keys 8 g + 0..7
    }
    // ---- O^T = V^T P^T (the wave's own LDS writes above are complete: same-wave LDS ops execute in order)
    __builtin_amdgcn_s_waitcnt(0xc07f);
    asm volatile("" ::: "memory");
    f32x4_t oacc[2][4];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) {
        const elem8_t vf = vt_frag<32>(Vt, dt * 16 + u, g);
#pragma unroll
        for (int qt = 0; qt < 2; ++qt) oacc[qt][dt] = VMV_MFMA16(vf, pf[qt], f32x4_t{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
    }
#pragma unroll
    for (int qt = 0; qt < 2; ++qt) {
        const int q = qt * 16 + u;
        if (q < p.Nq) store_o<4>(b.o + (long)q * p.om.s_row + 4 * g, oacc[qt], linv[qt]);
    }
}

int map_ok(const VmvSeqMap& m) {
    return m.inner > 0 && !(m.s_outer & 7) && !(m.s_inner & 7) && !(m.s_row & 3);
}

// The ONE host decision of this file: every argument check of vmv_attention and the choice between its seven kernels.  Returns the
// VMV_ATTN_* id of the kernel to launch, or the negative VMV_E* code; touches no device.  vmv_attention indexes its launch table with
// the result and vmv_attention_served_kernel returns it, so the two cannot disagree.
int attn_decide(const VmvAttnParams* pp) {
    if (!pp) return VMV_ENULL;
    const VmvAttnParams& p = *pp;
    if (!p.q || !p.k || !p.v || !p.o) return VMV_ENULL;
    if (p.n_outer <= 0 || p.heads <= 0 || p.Nq <= 0 || p.Nk <= 0 || p.kv_div <= 0) return VMV_EINVAL;
    {   // the kernels index the rows of one problem with 32-bit element offsets; the 4-waves-per-problem kernels issue K / V DMA
        // offsets for the whole last 64-row tile (rows >= Nk must land OUTSIDE the descriptor, i.e. must not wrap), and a row is
        // head_dim elements wide: validate the PADDED counts with the actual head_dim
        const long lim = 1L << 30;
        const long hdw = p.head_dim ? p.head_dim : 64;
        const long nq_pad = ((long)p.Nq + 255) / 256 * 256, nk_pad = ((long)p.Nk + 63) / 64 * 64;
        if ((nq_pad - 1) * p.qm.s_row + hdw >= lim || (nq_pad - 1) * p.om.s_row + hdw >= lim || (nk_pad - 1) * p.km.s_row + hdw >= lim ||
            (nk_pad - 1) * p.vm.s_row + hdw >= lim || p.qm.s_row < 0 || p.km.s_row < 0 || p.vm.s_row < 0 || p.om.s_row < 0) return VMV_ERANGE;
    }
    if (!map_ok(p.qm) || !map_ok(p.km) || !map_ok(p.vm) || !map_ok(p.om)) return VMV_EALIGN;
    if ((p.qm.s_row & 7) || (p.km.s_row & 7) || (p.vm.s_row & 7)) return VMV_EALIGN;
    if (!vmv_aligned16(p.q) || !vmv_aligned16(p.k) || !vmv_aligned16(p.v) || (((uintptr_t)p.o) & 7)) return VMV_EALIGN;
    const int hd = p.head_dim ? p.head_dim : 64;
    if (p.causal && (hd != 64 || p.Nq != p.Nk)) return VMV_EINVAL;          // causal: self-attention on the general head_dim-64 kernel
    const bool grid3 = p.n_outer <= 65535 && p.heads <= 65535;              // (query tile, head, problem) grid of the 4-waves-per-problem kernels
    if (hd == 32) return grid3 ? VMV_ATTN_D32 : VMV_ERANGE;                 // LGM MVAttention (core/attention.py:67-84): long sequences only
    if (hd == 128) return grid3 ? VMV_ATTN_D128 : VMV_ERANGE;               // zero-padded wide heads (the CLIP image tower's head_dim 80 packed to 128: clip_vision.py)
    if (hd != 64) return VMV_EINVAL;
    if (p.Nq <= 32 && p.Nk <= 32 && !p.causal) return VMV_ATTN_SHORT;
    if (p.Nq <= 32 && !p.causal) return VMV_ATTN_WAVE;
    if (!grid3) return VMV_ERANGE;
    if (p.causal) return VMV_ATTN_CAUSAL;
    // (round 6: 64-query blocks — QT = 1, 84 registers, four blocks per CU — for the short problems (Nk <= 192 or Nq <= 192: cross-
    //  attention, third-level / middle self-attention) measured step-neutral: 47.88 / 47.91 vs 47.86 / 47.87 ms, attention family
    //  4.16 / 4.13 vs 4.17 / 4.17 ms, profiles/r6_attn_q64_step_ab.log — not kept)
    // 256-query blocks when that still leaves >= 2 blocks per CU and the key loop is long enough to matter
    const long blocks256 = (long)((p.Nq + 255) / 256) * p.heads * p.n_outer;
    const bool big = p.Nk >= 512 && blocks256 >= 512 && (p.Nq % 256 == 0 || p.Nq >= 2048);
    return big ? VMV_ATTN_Q256 : VMV_ATTN_Q128;
}

// How each VMV_ATTN_* kernel is launched: queries per block (0: one problem per wave, four per block), dynamic LDS bytes, and
// whether that size has to be allowed first (once per device: vmv_lds_attr_once)
struct AttnLaunch {
    void (*kernel)(const VmvAttnParams, const int);
    int qblock, lds;
    bool lds_attr;
    std::atomic<unsigned long long> attr_done{0};
};
AttnLaunch attn_launch[] = {
    {},
    /* VMV_ATTN_SHORT  */ {attn_short_kernel, 0, 0, false},
    /* VMV_ATTN_WAVE   */ {attn_wave_kernel, 0, 4 * 8192, true},
    /* VMV_ATTN_Q128   */ {attn_block_kernel<2>, 128, attn_block_lds(64), false},
    /* VMV_ATTN_Q256   */ {attn_block_kernel<4>, 256, attn_block_lds(64), false},
    /* VMV_ATTN_CAUSAL */ {attn_block_kernel<2, 64, true>, 128, attn_block_lds(64), false},
    /* VMV_ATTN_D32    */ {attn_block_kernel<2, 32>, 128, attn_block_lds(32), false},
    /* VMV_ATTN_D128   */ {attn_block_kernel<2, 128>, 128, attn_block_lds(128), true},
};
static_assert(VMV_ATTN_SHORT == 1 && VMV_ATTN_WAVE == 2 && VMV_ATTN_Q128 == 3 && VMV_ATTN_Q256 == 4 && VMV_ATTN_CAUSAL == 5 &&
              VMV_ATTN_D32 == 6 && VMV_ATTN_D128 == 7 && sizeof(attn_launch) / sizeof(attn_launch[0]) == 8, "attn_launch is indexed by VMV_ATTN_*");

}  // namespace

extern "C" int vmv_attention_served_kernel(const VmvAttnParams* pp) { return attn_decide(pp); }

extern "C" int vmv_attention(const VmvAttnParams* pp, void* stream) {
    const int which = attn_decide(pp);
    if (which < 0) return which;
    const VmvAttnParams& p = *pp;
    AttnLaunch& l = attn_launch[which];
    if (l.lds_attr)
        if (const int rc_attr = vmv_lds_attr_once(l.attr_done, reinterpret_cast<const void*>(l.kernel), l.lds)) return rc_attr;
    const int nproblems = l.qblock ? 0 : p.n_outer * p.heads;
    const dim3 grid = l.qblock ? dim3((p.Nq + l.qblock - 1) / l.qblock, p.heads, p.n_outer) : dim3((nproblems + 3) / 4);
    hipLaunchKernelGGL(l.kernel, grid, dim3(256), l.lds, reinterpret_cast<hipStream_t>(stream), p, nproblems);
    return vmv_launch_status();
}
