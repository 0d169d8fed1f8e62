// Body of wino3x3_x3_kernel / wino3x3_x3_one_pass_kernel (csrc/conv_wino_x3_kernel.h, which tells the kernel's story and includes this file INSIDE each of the two
// kernels): not a header of its own.  In scope where it is included: the template parameters FUSE, UP, TX3, NT, NP, NEXT, SKD, W8, DMA, the constant ONEP and the
// kernel's argument `a`.
    static_assert(NT == 4 || (NT == 2 && !FUSE), "64-channel form: plain convolution only");
    static_assert(!DMA || (NP == 2 && !W8), "halo by LDS-DMA: the four-wave fp16 form");
    static_assert(!SKD || (DMA && FUSE && TX3 && UP && !NEXT), "skip rows by LDS-DMA: the LDS-DMA form's tail with the up-sampled addend (the form it measured faster on)");
    static_assert(!W8 || (NT == 4 && NP == 2 && !NEXT && (TX3 || !FUSE)), "eight waves: the fp16 form of the 128-channel kernel, without the next block's conv1");
    static_assert(!ONEP || (DMA && FUSE && TX3 && !UP && !SKD), "one-pass tail: the LDS-DMA form's plain tail and its tail with the next block's conv1");
    constexpr int NTHR = W8 ? 512 : 256;
    static_assert(!NEXT || (FUSE && TX3 && NP == 2), "the next block's conv1 rides on the fp16 tail");
    static_assert(NP == 3 || !FUSE || TX3, "the fp16 form's tail runs on the fp16 pipe");
    // one LDS array: halo double buffer (fp32) | V (three bf16 planes); the fused tail re-uses ALL of it for the conv2 tile
    constexpr int HSZ = X_NPIX * X_PKH;                       // floats per halo buffer
    constexpr int VROW = 16;                                  // bf16 per (tile, chunk) row = 32 bytes; the two 16-byte halves swap where bits 2 and 3 of the tile differ (4-7, 8-11, 20-23, 24-27):
                                                              // conflict-free A-fragment ds_read_b128, 2-way instead of 4-way on the transform's ds_write_b64
    constexpr int VPL = 16 * 32 * VROW;                       // bf16 per plane
    constexpr int VFLOATS = NP * VPL / 2;
    // (W8: one workgroup per CU anyway -- the tail's eight transposition patches get their own room behind the operand planes)
    constexpr int TAILF = NP * 8 * (64 * 32 + 32) / 4;        // floats of the tail's operand planes (NP planes x 8 k-steps x (64 pixels x 32 bytes + 32))
    constexpr int SKF = SKD ? 4 * 1024 : 0;                   // SKD: four 1 KiB skip-row slots per wave BEHIND everything else -- a DMA into them never meets the K loop's or the tail's own LDS
    constexpr int TAIL1F = NP * 8 * (128 * 32 + 32) / 4 + 4 * 16 * 36;      // ONEP: the whole tile's operand planes (128 pixels) and four HALF patches behind them
    constexpr int SFLOATS = W8 ? (2 * HSZ + VFLOATS > TAILF + 8 * 32 * 36 ? 2 * HSZ + VFLOATS : TAILF + 8 * 32 * 36)
                               : ONEP ? (2 * HSZ + VFLOATS > TAIL1F ? 2 * HSZ + VFLOATS : TAIL1F) : 2 * HSZ + VFLOATS + SKF;
    static_assert(SFLOATS * 4 <= 80 * 1024, "two workgroups per CU");
    __shared__ __attribute__((aligned(16))) float S[SFLOATS];
    float (*Hin)[HSZ] = reinterpret_cast<float (*)[HSZ]>(&S[0]);
    uint16_t* V = reinterpret_cast<uint16_t*>(&S[2 * HSZ]);
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int tiles_x = (a.OW + X_TW - 1) / X_TW, tiles_y = (a.OH + X_TH - 1) / X_TH;
    int bid = xcd_block_id();          // XCD-aware tile order (csrc/mma_ops.h)
    const int l = bid / (tiles_x * tiles_y);
    bid -= l * tiles_x * tiles_y;
    const int ty0 = bid / tiles_x, tx0 = bid - ty0 * tiles_x;
    const int oy0 = ty0 * X_TH, ox0 = tx0 * X_TW;
    const int iy0 = oy0 - 1, ix0 = ox0 - 1;
    const int nch = a.C / X_CK;
    const float* in_l = a.in + (size_t)l * a.H * a.W * a.C;
    const __amdgpu_buffer_rsrc_t in_srd = make_srd(in_l, (size_t)a.H * a.W * a.C * sizeof(float));
    const __amdgpu_buffer_rsrc_t w_srd = make_srd(a.Wp, (size_t)a.N * a.C * 16 * NP * sizeof(uint16_t));
    const __amdgpu_buffer_rsrc_t out_srd = make_srd(a.out + (size_t)l * a.OH * a.OW * a.N, (size_t)a.OH * a.OW * a.N * sizeof(float));

    // ---- halo staging (as csrc/conv_wino.hip): 180 pixels x 4 float4 per chunk over 256 threads -----------------------------
    constexpr int NF4 = X_NPIX * 4, NLD = (NF4 + NTHR - 1) / NTHR;
    constexpr int HP = DMA ? 16 : X_PKH;                      // floats per pixel of a halo buffer
    static_assert(!DMA || (NLD == 3 && NLD * NTHR * 4 <= HSZ), "LDS-DMA staging: three 1 KiB pieces per wave inside a halo buffer");
    int avoff[NLD];
#pragma unroll
    for (int i = 0; i < NLD; ++i) {
        const int idx = tid + i * NTHR;
        const int pix = idx >> 2;
        const int py = pix / X_IW, px = pix - py * X_IW;
        const int cc = DMA ? (idx & 3) ^ ((py >> 1) & 3) : idx & 3;      // DMA: slot idx holds this quad of the pixel (see the kernel's comment)
        const int iy = iy0 + py, ix = ix0 + px;
        const bool ok = idx < NF4 && iy >= 0 && iy < a.H && ix >= 0 && ix < a.W;
        avoff[i] = ok ? ((iy * a.W + ix) * a.C + cc * 4) * 4 : BUF_OOB;
    }
    // DMA: chunk c -> halo buffer buf, three pieces of 1 KiB per wave at float4 slots (256 i + 64 w) + lane.  M0 = the piece's LDS byte address, written and restored
    // inside the statement (hipcc reserves M0 and does not see it used here)
    const unsigned lds_w = __builtin_amdgcn_readfirstlane((unsigned)(size_t)&S[0]) + w * 1024;
    auto dma = [&](int c, int buf) {
        if constexpr (DMA) {
            const unsigned d0 = lds_w + buf * (HSZ * 4), d1 = d0 + NTHR * 16, d2 = d0 + 2 * NTHR * 16;
            const int soff = c * X_CK * 4;
            unsigned keep;
            asm volatile("s_mov_b32 %0, m0\n\t"
                         "s_nop 4\n\t"
                         "s_mov_b32 m0, %5\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %4, %8 offen lds\n\t"
                         "s_mov_b32 m0, %6\n\ts_nop 0\n\tbuffer_load_dwordx4 %2, %4, %8 offen lds\n\t"
                         "s_mov_b32 m0, %7\n\ts_nop 0\n\tbuffer_load_dwordx4 %3, %4, %8 offen lds\n\t"
                         "s_mov_b32 m0, %0"
                         : "=&s"(keep)
                         : "v"(avoff[0]), "v"(avoff[NLD > 1 ? 1 : 0]), "v"(avoff[NLD > 2 ? 2 : 0]), "s"(in_srd), "s"(d0), "s"(d1), "s"(d2), "s"(soff)
                         : "memory");
        }
    };
    f32x4 areg[NLD];
    auto gload = [&](int c) {
#pragma unroll
        for (int i = 0; i < NLD; ++i) areg[i] = buf_load(in_srd, avoff[i], c * X_CK * 4);
    };
    float dmax = 0.f;                                         // NP = 2: largest scaled input magnitude this lane staged (range guard)
    const float xs = NP == 2 ? s2_xscale(a.xscale) : 1.f;    // NP = 2: the input site's factor 2^s (uniform)
    auto sstore = [&](int buf) {
#pragma unroll
        for (int i = 0; i < NLD; ++i) {
            const int idx = tid + i * NTHR;
            if constexpr (NP == 2) {                              // the activation scale (exact) and the guard's running max ride on the staging copy
                areg[i] *= xs;
                dmax = s2_track(s2_track(dmax, areg[i][0], areg[i][1]), areg[i][2], areg[i][3]);
            }
            if (idx < NF4) *(f32x4*)&Hin[buf][(idx >> 2) * X_PKH + (idx & 3) * 4] = areg[i];
        }
    };
    auto dtrack = [&](int buf) {                              // DMA: the guard's running max over the lane's own slots of a landed buffer (unscaled: times xs at the end)
#pragma unroll
        for (int i = 0; i < NLD; ++i) {
            const f32x4 v = *(const f32x4*)&Hin[buf][(tid + i * NTHR) * 4];
            dmax = s2_track(s2_track(dmax, v[0], v[1]), v[2], v[3]);
        }
    };
    // ---- weights: Up3[(chunk * 16 + comp)][nb][plane][lane][8 bf16]: 3 KB per (component, n-tile), three 16-byte loads per lane -----
    // (128 output channels: NB = 4 n-tiles; the plane offset rides in the instruction's immediate field, one scalar addition per component.
    // The group offset is the instruction's SCALAR offset, which raw buffer loads do not range-check: every prefetch must name a group
    // inside Wq3 -- the loop below re-requests the last chunk's first pair instead of running past the end.)
    const int wvoff = lane * 16;
    const int wn = NT == 4 ? (W8 ? (w & 3) : w) : (w & 1), wc = NT == 4 ? (W8 ? (w >> 2) : 0) : (w >> 1);      // n-tile, component half
    constexpr bool HALF = NT == 2 || W8;                        // the wave owns half of the components, one accumulator each
    constexpr int NPAIR = HALF ? 4 : 8;                         // component pairs per chunk and wave
    const int wsbase = wn * NP * 1024;
    auto bload = [&](int gc, u32x4 (&b)[NP]) {              // gc = chunk * 16 + comp
        const int g = gc;
#pragma unroll
        for (int p = 0; p < NP; ++p) b[p] = __builtin_bit_cast(u32x4, buf_load(w_srd, wvoff + p * 1024, g * (NT * NP * 1024) + wsbase));
    };
    // ---- transform: thread = (tile tt, channel quad tq, half th) as in csrc/conv_wino.hip; every result vector is split on its way to LDS ----
    const int tt = tid & 31, tq = (tid >> 5) & 3, th = (tid >> 7) & 1;
    const int tv = __builtin_amdgcn_readfirstlane(tid >> 8);   // W8: which of the half's two rows this thread computes (0: first - third, 1: second +- other)
    const int t_ty = tt >> 3, t_tx = tt & 7;
    const int hbase = ((2 * t_ty + th) * X_IW + 2 * t_tx) * HP + (DMA ? (tq ^ t_ty) : tq) * 4;
    // DMA: the quad's slot is tq ^ ((R >> 1) & 3), R = the halo row: R >> 1 = t_ty for the thread's rows up to 2 t_ty + 1, t_ty + 1 for the rows from 2 t_ty + 2
    const int hbase1 = DMA ? ((2 * t_ty + th) * X_IW + 2 * t_tx) * HP + (tq ^ ((t_ty + 1) & 3)) * 4 : hbase;
    // V element offset of (component 0, tile tt, channels 4 tq ..): row tt, half (tq >> 1) swapped where bits 2, 3 of tt differ, 4 bf16 = 8 bytes
    const int vbase = tt * VROW + ((((tq >> 1) ^ (((tt >> 2) ^ (tt >> 3)) & 1)) * 8) + (tq & 1) * 4);
    auto vstore = [&](int comp, f32x4 v) {
        if constexpr (NP == 2) {
            split_store4<2, VPL>(&V[comp * 32 * VROW + vbase], v[0], v[1], v[2], v[3]);
            return;
        }
        // (NP = 3 keeps its own chain, the residuals as ONE vector subtraction: through split_store4's scalar form the bf16x3 kernels measured 1.3 - 1.6 % slower,
        //  profiles/mma_ops_header.txt.  Same values: round-to-nearest terms of csrc/bf16x3.h, the subtractions exact.)
#pragma unroll
        for (int p = 0; p < 3; ++p) {
            const unsigned q0 = s3_pack_rn(v[0], v[1]), q1 = s3_pack_rn(v[2], v[3]);
            *(u32x2*)&V[p * VPL + comp * 32 * VROW + vbase] = u32x2{q0, q1};
            if (p < 2) v = x_sub4(v, f32x4{s3_lo(q0), s3_hi(q0), s3_lo(q1), s3_hi(q1)});
        }
    };
    // rows of B^T d:  half 0 (input rows 0,1,2): xi0 = r0 - r2, xi1 = r1 + r2;  half 1 (rows 1,2,3): xi3 = r1 - r3, xi2 = r2 - r1
    // = (first - third, second +- other) with `other` = third / first row of the half's three: the row is picked by address, the sign is a scalar
    const int hother = th ? 0 : 2 * X_IW * HP;
    const float hsign = th ? -1.f : 1.f;
    auto transform = [&](int buf) {
        const float* hs = &Hin[buf][hbase];
        if constexpr (W8) {                                      // one row per thread: two of the four halo rows, four components
            const int xi = tv == 0 ? (th ? 3 : 0) : (th ? 2 : 1);
            f32x4 e[4];
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                if (tv == 0) {
                    e[c] = x_sub4(*(const f32x4*)(hs + c * X_PKH), *(const f32x4*)(hs + (2 * X_IW + c) * X_PKH));
                } else {
                    const f32x4 l1 = *(const f32x4*)(hs + (X_IW + c) * X_PKH), lx = *(const f32x4*)(hs + hother + c * X_PKH);
                    e[c] = f32x4{__builtin_fmaf(lx[0], hsign, l1[0]), __builtin_fmaf(lx[1], hsign, l1[1]), __builtin_fmaf(lx[2], hsign, l1[2]), __builtin_fmaf(lx[3], hsign, l1[3])};
                }
            }
            vstore(xi * 4 + 0, x_sub4(e[0], e[2]));
            vstore(xi * 4 + 1, x_add4(e[1], e[2]));
            vstore(xi * 4 + 2, x_sub4(e[2], e[1]));
            vstore(xi * 4 + 3, x_sub4(e[1], e[3]));
            return;
        }
        // (DMA: rows 0 / 2 of the thread's three are in the slots of hbase / hbase1, the middle row and `other` in those of one each, by the half)
        const float* hs2 = &Hin[buf][hbase1];
        const float* hs1 = th ? hs2 : hs;
        const float* hsx = th ? hs : hs2;
        f32x4 L0[4], L1[4], L2[4], Lx[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            L0[c] = *(const f32x4*)(hs + c * HP);
            L1[c] = *(const f32x4*)(hs1 + (X_IW + c) * HP);
            L2[c] = *(const f32x4*)(hs2 + (2 * X_IW + c) * HP);
            Lx[c] = *(const f32x4*)(hsx + hother + c * HP);
        }
        f32x4 eA[4], eB[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            eA[c] = x_sub4(L0[c], L2[c]);
            eB[c] = f32x4{__builtin_fmaf(Lx[c][0], hsign, L1[c][0]), __builtin_fmaf(Lx[c][1], hsign, L1[c][1]), __builtin_fmaf(Lx[c][2], hsign, L1[c][2]),
                            __builtin_fmaf(Lx[c][3], hsign, L1[c][3])};                      // (a product by +-1 is exact: with or without contraction the same value)
            if constexpr (DMA) { eA[c] *= xs; eB[c] *= xs; }                                 // the site's 2^s, exact: the register path applies it to the staged elements
        }
        const int xiA = th ? 3 : 0, xiB = th ? 2 : 1;
        // columns: nu0 = c0 - c2, nu1 = c1 + c2, nu2 = c2 - c1, nu3 = c1 - c3
        vstore(xiA * 4 + 0, x_sub4(eA[0], eA[2]));
        vstore(xiA * 4 + 1, x_add4(eA[1], eA[2]));
        vstore(xiA * 4 + 2, x_sub4(eA[2], eA[1]));
        vstore(xiA * 4 + 3, x_sub4(eA[1], eA[3]));
        vstore(xiB * 4 + 0, x_sub4(eB[0], eB[2]));
        vstore(xiB * 4 + 1, x_add4(eB[1], eB[2]));
        vstore(xiB * 4 + 2, x_sub4(eB[2], eB[1]));
        vstore(xiB * 4 + 3, x_sub4(eB[1], eB[3]));
    };

    f32x16 zero16;
#pragma unroll
    for (int r = 0; r < 16; ++r) zero16[r] = 0.f;
    f32x16 out[4], Z[8];
#pragma unroll
    for (int p = 0; p < 4; ++p)
#pragma unroll
        for (int r = 0; r < 16; ++r) out[p][r] = 0.f;
#pragma unroll
    for (int p = 0; p < 8; ++p)
#pragma unroll
        for (int r = 0; r < 16; ++r) Z[p][r] = 0.f;
    // the cross terms of a component (six, or three for NP = 2), smallest first
    auto mac6 = [&](f32x16& acc, const bf16x8 (&f)[NP], const u32x4 (&bw)[NP], bool from_zero) {
#pragma unroll
        for (int t = 0; t < split_terms<NP>(); ++t) acc = split_mma<NP>(t, f, bw, (t == 0 && from_zero) ? zero16 : acc);
    };
    // Consumption order of the components, in pairs: pairs 0-3 = (xi 0, xi 3) of nu = pair, accumulated straight into their Z; pairs 4-7 =
    // (xi 1, xi 2) of nu = pair - 4, through two scratch accumulators that are folded into Z[0][nu], Z[1][nu].  The weights of pair p + 1
    // are requested before pair p's MFMAs.  Measured alternatives, all slower (tools/bench_wino_x3.py, 256 crops, plain / fused, us):
    // this schedule 920 / 1620; the two accumulation chains of a pair interleaved 1030 / 1800; one component at a time with the A
    // fragments one and the weights one / three components ahead 943 / 1690 and 1052 / 1825.
    auto comp_of = [&](int pair, int which) -> int {
        if (!HALF) return pair < 4 ? (which ? 12 + pair : pair) : (which ? 8 + (pair - 4) : 4 + (pair - 4));
        return wc * 8 + 2 * pair + which;                     // (64-channel form / eight waves: the wave's own half, in order)
    };
    // A operand of component comp: tile = lane & 31, channels 8 (lane >> 5) .. + 7 (the half, swapped as the rows were written)
    const int afoff = (lane & 31) * VROW + (((lane >> 5) ^ (((lane >> 2) ^ (lane >> 3)) & 1)) * 8);
    u32x4 bring[2][2][NP];                                  // [slot][which][plane]
    if constexpr (DMA) {
#pragma unroll
        for (int i = 0; i < NLD; ++i)                         // the slots no DMA of this lane ever fills (pixels outside the map, the pad behind slot 719), in both buffers
            if (avoff[i] == BUF_OOB) {
                *(f32x4*)&Hin[0][(tid + i * NTHR) * 4] = f32x4{0.f, 0.f, 0.f, 0.f};
                *(f32x4*)&Hin[1][(tid + i * NTHR) * 4] = f32x4{0.f, 0.f, 0.f, 0.f};
            }
        dma(0, 0);
    } else {
        gload(0);
    }
    bload(comp_of(0, 0), bring[0][0]);
    bload(comp_of(0, 1), bring[0][1]);
    if constexpr (DMA) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // chunk 0 has landed (and, once, the first pair's weights)
    else sstore(0);
    __syncthreads();

#ifdef SUO_WX3_PROF
    long long pt[5] = {0, 0, 0, 0, 0}, p0 = clock64();
#define XPROF(i) do { const long long _t = clock64(); pt[i] += _t - p0; p0 = _t; } while (0)
#else
#define XPROF(i) do { } while (0)
#endif
    for (int c = 0; c < nch; ++c) {
        const int buf = c & 1;
        const bool more = c + 1 < nch;
        if (more) {
            if constexpr (DMA) dma(c + 1, buf ^ 1);
            else gload(c + 1);
        }
        transform(buf);
        if constexpr (DMA) dtrack(buf);
        XPROF(0);
        __syncthreads();
        XPROF(1);
        if (more && !DMA) sstore(buf ^ 1);
        XPROF(2);
#pragma unroll
        for (int pair = 0; pair < NPAIR; ++pair) {
            const int slot = pair & 1;
            {   // next pair (of this chunk, or pair 0 of the next one; after the last chunk pair 0 of that chunk again -- never consumed, but in range)
                const int np = pair + 1 < NPAIR ? pair + 1 : 0, nc = pair + 1 < NPAIR ? c : (more ? c + 1 : c);
                bload(nc * 16 + comp_of(np, 0), bring[slot ^ 1][0]);
                bload(nc * 16 + comp_of(np, 1), bring[slot ^ 1][1]);
            }
            const int ca = comp_of(pair, 0), cb = comp_of(pair, 1);
            bf16x8 afa[NP], afb[NP];
#pragma unroll
            for (int p = 0; p < NP; ++p) {
                afa[p] = *(const bf16x8*)&V[p * VPL + ca * 32 * VROW + afoff];
                afb[p] = *(const bf16x8*)&V[p * VPL + cb * 32 * VROW + afoff];
            }
            __builtin_amdgcn_sched_barrier(0);
            if (HALF) {                                       // Z[local component]
                mac6(Z[2 * pair], afa, bring[slot][0], false);
                mac6(Z[2 * pair + 1], afb, bring[slot][1], false);
            } else if (pair < 4) {                            // accumulate into their own Z, no scratch, no additions
                mac6(Z[pair], afa, bring[slot][0], false);
                mac6(Z[4 + pair], afb, bring[slot][1], false);
            } else {
                f32x16 ta, tb;
                mac6(ta, afa, bring[slot][0], true);
                mac6(tb, afb, bring[slot][1], true);
                x_add16(Z[pair - 4], ta); x_add16(Z[pair - 4], tb); x_add16(Z[pair], ta); x_sub16(Z[pair], tb);      // Z[0][nu] += M1 + M2, Z[1][nu] += M1 - M2
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        XPROF(3);
        if constexpr (DMA) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");      // chunk c + 1 has landed; the next pair's four weight loads stay in flight
        __syncthreads();
        XPROF(4);
    }
    if constexpr (DMA) dmax *= xs;
#ifdef SUO_WX3_PROF
    if (blockIdx.x == 1000 && (tid & 63) == 0) printf("wave %d cycles: transform %lld  barrier1 %lld  sstore %lld  mfma+fold %lld  barrier2 %lld\n", w, pt[0], pt[1], pt[2], pt[3], pt[4]);
#endif
    if constexpr (NP == 2) s2_raise(a.range_flag, 4.f * dmax);    // |B^T d B| <= 4 max |d|: conservative by at most 4x, never late
    // second step of the output transform: R[h][j] = sum_nu A^T[j][nu] Z[4 h + nu].  128-channel form: h = i, R = Y; 64-channel form: h = the wave's local row
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        out[2 * h] = Z[4 * h] + Z[4 * h + 1] + Z[4 * h + 2];
        out[2 * h + 1] = Z[4 * h + 1] - Z[4 * h + 2] - Z[4 * h + 3];
    }
    // W8: the two component halves of an n-tile meet (as in the 64-channel form below): wave wc = 0 holds R of rows xi = 0, 1 (out[0..1], out[2..3]), wave wc = 1 of
    // rows 2, 3 (row 3 negated in the weights).  Y[0][j] = (R0 + R1) + R2, Y[1][j] = (R3' - R2) + R1: wave wc keeps output row i = wc and hands its MIDDLE row to the
    // partner through the V area ([wave][register][lane]: 32 KB per column j, two rounds)
    f32x16 mine[2];
    if constexpr (W8) {
        static_assert(VFLOATS >= 8 * 16 * 64, "the exchange area is the V planes");
        float* X = &S[2 * HSZ];                                // (the last chunk's closing barrier has passed: V is free)
        const int pw = (1 - wc) * 4 + wn;
#pragma unroll
        for (int q = 0; q < 2; ++q) {
#pragma unroll
            for (int r = 0; r < 16; ++r) X[(w * 16 + r) * 64 + lane] = wc == 0 ? out[2 + q][r] : out[q][r];
            __syncthreads();
#pragma unroll
            for (int r = 0; r < 16; ++r) mine[q][r] = (wc == 0 ? out[q][r] + out[2 + q][r] : out[2 + q][r] - out[q][r]) + X[(pw * 16 + r) * 64 + lane];
            __syncthreads();
        }
    }

    if constexpr (FUSE && TX3 && ONEP) {
        // ---- the tail in ONE pass over the tile (two fp16 planes: the whole 128-pixel conv2 tile is 66 048 B of operand, where the three bf16 planes that the
        // two passes below date from are 96 KB).  Every lane splits all four out[p] up front into AP[plane][k-step][pixel m of 128][16 channels], m = 64 h + (the pass
        // form's m): m-tiles 0, 1 are the pixel rows of parity 0, m-tiles 2, 3 those of parity 1 -- addresses, swaps and epilogue arithmetic are the pass form's with
        // i -> 2 h + i.  conv3 is ONE k-loop of 8 steps, 4 m-tiles x 2 n-tiles per wave: 24 MFMAs against the same four weight loads, W3 (and, NEXT, the next
        // block's W1) streamed once per tile instead of once per pass.  The transposition patches are HALF patches (16 rows x 36 floats per wave): accumulator
        // registers r < 8 are exactly rows 0-15 of the 32 x 32 block, r >= 8 rows 16-31 (acc_row), and the row groups k = 0, 1 / 2, 3 read those same halves, so a
        // block goes through its patch in two rounds.  75 264 B per workgroup: two per CU.  Every output element is the same sum of the same products in ascending
        // k, scale / bias / skip / NEXT prologue arithmetic unchanged: bit for bit the pass form's results, and the guard's maximum is over the same values.
        constexpr int KS_STRIDE = 128 * 32 + 32;                // bytes per k-step image (+ 32: the two k-steps a wave stores to hit different banks)
        constexpr int PL_STRIDE = 8 * KS_STRIDE;
        static_assert(NP == 2 && !W8 && NP * PL_STRIDE / 4 + 4 * 16 * 36 == TAIL1F && TAIL1F <= SFLOATS, "one-pass tail staging must fit the workgroup's LDS");
        // (the lane id from here on is opaque to hipcc: what the tail derives from it is then computed here, not ahead of the K loop, which has no register for it)
        int ln = lane;
        asm volatile("" : "+v"(ln));
        unsigned char* AP = reinterpret_cast<unsigned char*>(&S[0]);
        float* T = &S[NP * PL_STRIDE / 4] + w * (16 * 36);
        const __amdgpu_buffer_rsrc_t w3_srd = make_srd(a.W3p, (size_t)a.N * a.N2 * NP * sizeof(uint16_t));
        const size_t crop2 = (size_t)a.OH * a.OW * a.N2;
        const __amdgpu_buffer_rsrc_t r_srd = make_srd(a.R + (size_t)l * crop2, crop2 * sizeof(float));
        const __amdgpu_buffer_rsrc_t o2_srd = make_srd(a.out2 + (size_t)l * crop2, crop2 * sizeof(float));
        const float xs3 = s2_xscale(a.xscale3);
        const float b2v = a.bias[w * 32 + (ln & 31)] * xs3;
        const float c2v = a.oscale[w * 32 + (ln & 31)] * xs3;
        float tmax = 0.f;
        // (store and A-operand addresses: the pass form's, see there)
        const int sbase = (2 * w + ((ln >> 4) & 1)) * KS_STRIDE + (ln >> 5) * (8 * 32) + ((((ln >> 3) & 1) ^ (ln >> 5)) * 16) + (ln & 7) * 2;
        const int aoff = (ln & 31) * 32 + (((ln >> 5) ^ ((ln >> 3) & 1)) * 16);
        const int w3voff = ln * 16;
        auto b3load = [&](int ks, u32x4 (&b)[2][NP]) {
            const int k = ks < 8 ? ks : 7;
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int p = 0; p < NP; ++p) b[j][p] = __builtin_bit_cast(u32x4, buf_load(w3_srd, w3voff, (((k * 8 + 4 * j + w) * NP) + p) * 1024));
        };
        u32x4 b3[2][2][NP];
        b3load(0, b3[0]);
#pragma unroll
        for (int p = 0; p < 4; ++p)                           // output position p = 2 h + pj
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float v = fmaxf(fmaf(out[p][r], c2v, b2v), 0.f);
                const int off = sbase + (64 * (p >> 1) + 16 * (r >> 2) + 2 * (r & 3) + (p & 1)) * 32;
                tmax = fmaxf(tmax, v);                            // (v >= 0)
                const _Float16 hi = (_Float16)v, lo = (_Float16)(v - (float)hi);
                *reinterpret_cast<_Float16*>(AP + off) = hi;
                *reinterpret_cast<_Float16*>(AP + PL_STRIDE + off) = lo;
            }
        asm volatile("" : "+v"(tmax));                        // (the maximum is taken HERE: hipcc otherwise carries operands of it across conv3's loop, spilled)
        __syncthreads();
        f32x16 acc2[4][2];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) acc2[i][j] = zero16;
        // A fragments: two m-tiles (a half-step: 12 MFMAs of conv3, 6 of the next conv1) at a time, requested ONE HALF-STEP AHEAD of the MFMAs that consume them
        // -- all four m-tiles at once are 16 registers more than the kernel has beside acc2 and the weight ring.  half-step t = 2 (k-step) + (m-tile pair)
        auto afload = [&](int t, bf16x8 (&f)[2][NP]) {
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int p = 0; p < NP; ++p) f[i][p] = *(const bf16x8*)(AP + p * PL_STRIDE + (t >> 1) * KS_STRIDE + (2 * (t & 1) + i) * 1024 + aoff);
        };
        bf16x8 af[2][2][NP];
        afload(0, af[0]);
#pragma unroll
        for (int t = 0; t < 16; ++t) {
            const int ks = t >> 1, ih = t & 1;
            if (ih == 0) b3load(ks + 1, b3[(ks + 1) & 1]);
            if (t + 1 < 16) afload(t + 1, af[(t + 1) & 1]);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) mac6(acc2[2 * ih + i][j], af[t & 1][i], b3[ks & 1][j], false);
            __builtin_amdgcn_sched_barrier(0);
        }
        if constexpr (NEXT) __syncthreads();                  // every wave is past its conv3 reads of AP: the NEXT conv1's operand planes overwrite it
        f32x16 acc1[4];                                       // NEXT: conv1 of the next block, 128 pixels x channels [32 w, 32 w + 32) (first product block from zero)
        // one 32 x 32 block through the wave's half patch: round g = accumulator registers 8 g .. 8 g + 7 = rows 16 g .. 16 g + 15 = row groups k = 2 g, 2 g + 1
        auto half_rows = [&](const f32x16& acc, int g) {
#pragma unroll
            for (int r = 0; r < 8; ++r) T[acc_row(r, ln) * 36 + (ln & 31)] = acc[8 * g + r];
        };
#pragma unroll
        for (int j = 0; j < 2; ++j) {                         // j = the wave's n-tile: output channels [128 j + 32 w, + 32); NEXT: round j = conv1's K half j
            // (NEXT: the lane's pixel row is made opaque per round -- hipcc would otherwise keep the 16 blocks' pixel offsets of round 0 for round 1 and for
            //  conv1's epilogue, across the K halves where the kernel has no register to spare: 44 spilled.  Recomputing them is a few integer operations a row.)
            int lrow = ln >> 3;
            if constexpr (NEXT) asm volatile("" : "+v"(lrow));
#pragma unroll
            for (int i = 0; i < 4; ++i) {                     // m-tile i: pass-form pass h = i >> 1, its m-tile i & 1
                const int col = (4 * j + w) * 32 + (ln & 7) * 4;
                const f32x4 bv = *(const f32x4*)(a.bias3 + col);
                const f32x4 osc3 = *(const f32x4*)(a.oscale3 + col);
                f32x4 nsc, nsh;
                if constexpr (NEXT) { const float nxs = s2_xscale(a.n_xscale); nsc = *(const f32x4*)(a.n_scale + col) * nxs; nsh = *(const f32x4*)(a.n_shift + col) * nxs; }
                int off[4];
                f32x4 rv[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int m = 32 * (i & 1) + lrow + 8 * k;
                    const int oy = oy0 + 2 * (m >> 4) + (i >> 1), ox = ox0 + (m & 15);
                    off[k] = (oy < a.OH && ox < a.OW) ? ((oy * a.OW + ox) * a.N2 + col) * 4 : BUF_OOB;
                    rv[k] = buf_load(r_srd, off[k], 0);
                }
#pragma unroll
                for (int g = 0; g < 2; ++g) {
                    half_rows(acc2[i][j], g);
                    __builtin_amdgcn_wave_barrier();
#pragma unroll
                    for (int k = 2 * g; k < 2 * g + 2; ++k) {
                        f32x4 o = *(const f32x4*)&T[((ln >> 3) + 8 * (k - 2 * g)) * 36 + (ln & 7) * 4];
                        o *= osc3;                                // back to scale (an exact power of two per column)
                        o = (o + bv) + rv[k];
                        buf_store(o, o2_srd, off[k]);
                        if constexpr (NEXT) {
                            // the next block's operand (the pass form's, see there), pixel m of the 128
                            const int m = 32 * i + lrow + 8 * k;
                            float xn[4];
#pragma unroll
                            for (int c = 0; c < 4; ++c) xn[c] = fmaxf(fmaf(o[c], nsc[c], nsh[c]), 0.f);
                            tmax = fmaxf(fmaxf(tmax, fmaxf(xn[0], xn[1])), fmaxf(xn[2], xn[3]));
                            unsigned char* d = AP + (2 * w + ((ln & 7) >> 2)) * KS_STRIDE + m * 32 + (((((ln & 3) >> 1) ^ ((m >> 3) & 1))) * 16) + (ln & 1) * 8;
                            split_store4<2, PL_STRIDE>(d, xn[0], xn[1], xn[2], xn[3]);
                        }
                    }
                    __builtin_amdgcn_wave_barrier();
                }
                if constexpr (NEXT) {                         // (with the next conv1's accumulators live, skip rows requested blocks ahead or operands of the
                    asm volatile("" : "+v"(tmax));            //  guard's maximum carried across a K half would spill)
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
            if constexpr (NEXT) {
                // K half j of conv1 (k-steps 8 j .. 8 j + 7, ascending: the order of gemm_bf16x3_kernel) over all 128 pixels: wave w -> n-tile w, 12 MFMAs per k-step
                const __amdgpu_buffer_rsrc_t n1_srd = make_srd(a.n_W1, (size_t)128 * 256 * 2 * sizeof(uint16_t));
                auto n1load = [&](int q, u32x4 (&b)[2]) {
                    const int ksg = 8 * j + (q < 8 ? q : 7);
#pragma unroll
                    for (int p = 0; p < 2; ++p) b[p] = __builtin_bit_cast(u32x4, buf_load(n1_srd, w3voff + p * 1024, ((ksg * 4 + w) * 2) * 1024));
                };
                constexpr int NR = 3;                         // weight k-steps in flight (12 MFMAs = 384 cycles a k-step)
                u32x4 nb[NR][2];
#pragma unroll
                for (int q = 0; q < NR - 1; ++q) n1load(q, nb[q]);
                __syncthreads();                              // the four waves' planes of this K half are complete
                afload(0, af[0]);
#pragma unroll
                for (int t = 0; t < 16; ++t) {                // (half-steps, as in conv3's loop)
                    const int q = t >> 1, ih = t & 1;
                    if (ih == 0) n1load(q + NR - 1, nb[(q + NR - 1) % NR]);
                    if (t + 1 < 16) afload(t + 1, af[(t + 1) & 1]);
                    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                    for (int i = 0; i < 2; ++i) mac6(acc1[2 * ih + i], af[t & 1][i], nb[q % NR], j == 0 && q == 0);
                    __builtin_amdgcn_sched_barrier(0);
                }
                if (j == 0) __syncthreads();                  // every wave has read the planes: the next K half may overwrite them
            }
        }
        if constexpr (NEXT) {
            // conv1's epilogue as gemm_bf16x3_kernel's: acc * oscale + bias, ReLU, 16-byte stores of the wave's 32 channels of the 128 pixels
            asm volatile("" : "+v"(ln));                      // (as at the tail's top: nothing of this epilogue is carried across the K halves)
            const int col = w * 32 + (ln & 7) * 4;
            const f32x4 b1 = *(const f32x4*)(a.n_b1 + col), o1 = *(const f32x4*)(a.n_osc1 + col);
            const size_t cropn = (size_t)a.OH * a.OW * 128;
            const __amdgpu_buffer_rsrc_t n_srd = make_srd(a.n_out + (size_t)l * cropn, cropn * sizeof(float));
            int lrow = ln >> 3;
            asm volatile("" : "+v"(lrow));                    // (as above)
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int g = 0; g < 2; ++g) {
                    half_rows(acc1[i], g);
                    __builtin_amdgcn_wave_barrier();
#pragma unroll
                    for (int k = 2 * g; k < 2 * g + 2; ++k) {
                        const int m = 32 * (i & 1) + lrow + 8 * k;
                        const int oy = oy0 + 2 * (m >> 4) + (i >> 1), ox = ox0 + (m & 15);
                        f32x4 o = *(const f32x4*)&T[((ln >> 3) + 8 * (k - 2 * g)) * 36 + (ln & 7) * 4];
                        o *= o1;
                        o += b1;
#pragma unroll
                        for (int c = 0; c < 4; ++c) o[c] = fmaxf(o[c], 0.f);
                        buf_store(o, n_srd, (oy < a.OH && ox < a.OW) ? ((oy * a.OW + ox) * 128 + col) * 4 : BUF_OOB);
                    }
                    __builtin_amdgcn_wave_barrier();
                }
        }
        s2_raise(a.range_flag, tmax);
        return;
    }

    if constexpr (FUSE && TX3 && !ONEP) {
        // ---- tail of the Residual block (layers/Residual.py:27-35) on the bf16 pipe as well: out2 = W3 relu(conv2 + bias2) + bias3 + skip [+ up],
        // conv3 = 1x1, 128 -> 256.  The conv2 tile (128 pixels x 128 channels, in `out`: wave w holds channels [32 w, 32 w + 32) as 4 output
        // positions x 32 Winograd tiles) is the A operand; split into three bf16 planes it is 96 KB, so it goes through LDS in two halves of
        // 64 pixels: pass h = the output positions of pixel row parity h (image rows oy0 + 2 ty + h).  Per pass: every lane splits its 32
        // values and stores the bf16 terms (round-to-nearest of the value and of its two exact residuals: ds_write_b16_d16_hi) into
        // AP[plane][k-step][pixel m = 16 ty + x][16 channels] (A-operand order: 32-byte rows, the 16-byte halves swapped for pixels 8-15 of
        // every 16); barrier; wave w computes the 64 pixels x output channels [64 w, 64 w + 64) (2 x 2 accumulators, 8 k-steps x 24 MFMAs),
        // then its epilogue (transposition through a wave-private patch, + bias3 + skip [+ up], 16-byte stores).
        constexpr int KS_STRIDE = 64 * 32 + 32;                 // bytes per k-step image (+ 32: the two k-steps a wave stores to hit different banks)
        constexpr int PL_STRIDE = 8 * KS_STRIDE;
        static_assert(NP * PL_STRIDE == TAILF * 4 && NP * PL_STRIDE + (W8 ? 8 : 4) * 32 * 36 * 4 <= SFLOATS * 4, "tail staging must fit the workgroup's LDS");
        constexpr int NJ = W8 ? 1 : 2;                          // n-tiles of conv3 per wave: W8 -> the one tile w of eight; else tiles w and 4 + w
        unsigned char* AP = reinterpret_cast<unsigned char*>(&S[0]);
        float* T = &S[NP * PL_STRIDE / 4] + w * (32 * 36);
        const __amdgpu_buffer_rsrc_t w3_srd = make_srd(a.W3p, (size_t)a.N * a.N2 * NP * sizeof(uint16_t));
        const size_t crop2 = (size_t)a.OH * a.OW * a.N2;
        const __amdgpu_buffer_rsrc_t r_srd = make_srd(a.R + (size_t)l * crop2, crop2 * sizeof(float));
        const __amdgpu_buffer_rsrc_t o2_srd = make_srd(a.out2 + (size_t)l * crop2, crop2 * sizeof(float));
        constexpr bool has_up = UP;
        const __amdgpu_buffer_rsrc_t up_srd = make_srd(has_up ? a.up + (size_t)l * (crop2 / 4) : a.R, has_up ? crop2 / 4 * sizeof(float) : 0);
        // NP = 2: the conv2 accumulator carries 2^(t_n + s); conv3's operand is 2^s3 relu(conv2 + b2) = relu(acc 2^-(t_n + s) 2^s3 + 2^s3 b2): one fma
        // (s, s3: the sites of conv2's and conv3's inputs; both factors exact powers of two)
        const float xs3 = NP == 2 ? s2_xscale(a.xscale3) : 1.f;
        const float b2v = NP == 2 ? a.bias[wn * 32 + (lane & 31)] * xs3 : a.bias[wn * 32 + (lane & 31)];
        const float c2v = NP == 2 ? a.oscale[wn * 32 + (lane & 31)] * xs3 : 1.f;
        float tmax = 0.f;
        // store address of the lane's channel n = 32 w + (lane & 31): k-step n >> 4, half (n >> 3) & 1 (swapped for pixels 8-15: = lane >> 5, see m below),
        // element n & 7; pixel m = 16 (r >> 2) + 2 (r & 3) + 8 (lane >> 5) + pj for accumulator row r (tile (r & 3) + 8 (r >> 2) + 4 (lane >> 5))
        const int sbase = (2 * wn + ((lane >> 4) & 1)) * KS_STRIDE + (lane >> 5) * (8 * 32) + ((((lane >> 3) & 1) ^ (lane >> 5)) * 16) + (lane & 7) * 2;
        // A operand: pixel m = 32 i + (lane & 31), channels 8 (lane >> 5) .. + 7 of the k-step
        const int aoff = (lane & 31) * 32 + (((lane >> 5) ^ ((lane >> 3) & 1)) * 16);
        // weights: W3x[(ks * 8 + nb) * 3 + plane][lane][8 bf16], 1 KB each (pack_tail_weight_bf16x3); the wave's n-tiles are w and 4 + w (output channels
        // [32 w, 32 w + 32) and [128 + 32 w, ...): the four waves' first tiles are channels 0-127 in order, which is the K order the NEXT conv1 consumes them in)
        const int w3voff = lane * 16;
        // SKD: the skip rows by LDS-DMA (the kernel's comment).  Epilogue blocks in the order they run: b = 4 h + 2 j + i; slot k of the wave's buffer holds the 64 lanes'
        // 16 bytes of row group k of ONE block at a time.  skoff = the lane's byte offset inside the crop's 256-channel tensors (skip, out2), BUF_OOB outside the map:
        // the value of the epilogue's off[k] (pixel m = 32 i + (lane >> 3) + 8 k: row 2 (m >> 4) + h = 2 (2 i + (k >> 1)) + h and column (lane >> 3) + 8 (k & 1) of the
        // tile, channel 128 j + 32 w + 4 (lane & 7)) as ONE per-lane term plus wave-uniform ones: asking for the next block's offsets costs an addition and a select, no live registers
        const int sk_lane = ((oy0 * a.OW + ox0 + (lane >> 3)) * a.N2 + w * 32 + (lane & 7) * 4) * 4;
        auto skoff = [&](int b, int k) -> int {
            const int row = 2 * (2 * (b & 1) + (k >> 1)) + (b >> 2);
            const int xlim = oy0 + row < a.OH ? a.OW - ox0 - 8 * (k & 1) : 0;          // (uniform) the lanes with (lane >> 3) < xlim are inside the map
            const int lin = sk_lane + ((row * a.OW + 8 * (k & 1)) * a.N2 + 128 * ((b >> 1) & 1)) * 4;
            return (lane >> 3) < xlim ? lin : BUF_OOB;
        };
        const float* RB = &S[2 * HSZ + VFLOATS] + w * 1024;
        const unsigned rb_w = __builtin_amdgcn_readfirstlane((unsigned)(size_t)&S[2 * HSZ + VFLOATS]) + w * 4096;
        // one wave-instruction: row group k of block b -> slot k.  lgkmcnt(0) first: the lane's own ds_read_b128 of the slot's previous content (issued before this
        // statement) has returned before the DMA can overwrite it.  M0 as in the halo's statement
        auto skdma = [&](int b, int k) {
            if constexpr (SKD) {
                unsigned keep;
                asm volatile("s_waitcnt lgkmcnt(0)\n\t"
                             "s_mov_b32 %0, m0\n\t"
                             "s_nop 4\n\t"
                             "s_mov_b32 m0, %3\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, 0 offen lds\n\t"
                             "s_mov_b32 m0, %0"
                             : "=&s"(keep)
                             : "v"(skoff(b, k)), "s"(r_srd), "s"(rb_w + k * 1024)
                             : "memory");
            }
        };
        auto skwait = [&](int n) {                            // n folds to a constant in the unrolled epilogue
            switch (n) {
                case 3: asm volatile("s_waitcnt vmcnt(3)" ::: "memory"); break;
                case 4: asm volatile("s_waitcnt vmcnt(4)" ::: "memory"); break;
                case 5: asm volatile("s_waitcnt vmcnt(5)" ::: "memory"); break;
                case 6: asm volatile("s_waitcnt vmcnt(6)" ::: "memory"); break;
                default: asm volatile("s_waitcnt vmcnt(7)" ::: "memory"); break;
            }
        };
        // SKD: the epilogue's per-column vectors come from LDS (staged here once, in the 9.6 KB the tail leaves free behind its patches; visible after pass 0's barrier).
        // A load that hipcc counts, issued while a DMA is in flight, is waited for with a count that does not know of the DMA: its vmcnt(0) drained the DMA of the block ahead
        float* CB = &S[NP * PL_STRIDE / 4 + 4 * 32 * 36];
        if constexpr (SKD) {
            static_assert(NP * PL_STRIDE + 4 * 32 * 36 * 4 + 2 * 256 * 4 <= (2 * HSZ + VFLOATS) * 4 && NTHR == 256, "column vectors: 256 threads, one column each");
            CB[tid] = a.bias3[tid];
            CB[256 + tid] = a.oscale3[tid];
#pragma unroll
            for (int k = 0; k < 4; ++k) skdma(0, k);         // block 0: under pass 0's operand split (the conv3 k-loop's first counted wait for its weights retires it too)
        }
        auto b3load = [&](int ks, u32x4 (&b)[2][NP]) {
            const int k = ks < 8 ? ks : 7;
#pragma unroll
            for (int j = 0; j < NJ; ++j)
#pragma unroll
                for (int p = 0; p < NP; ++p) b[j][p] = __builtin_bit_cast(u32x4, buf_load(w3_srd, w3voff, (((k * 8 + (W8 ? w : 4 * j + w)) * NP) + p) * 1024));
        };
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            u32x4 b3[2][2][NP];
            b3load(0, b3[0]);
            if (!W8 || wc == h)                               // (W8: the pass's pixel rows are held by the waves of component half h)
#pragma unroll
            for (int pj = 0; pj < 2; ++pj)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const float cv = W8 ? mine[pj][r] : out[2 * h + pj][r];
                    float v = NP == 2 ? fmaxf(fmaf(cv, c2v, b2v), 0.f) : fmaxf(cv + b2v, 0.f);
                    const int off = sbase + (16 * (r >> 2) + 2 * (r & 3) + pj) * 32;
                    if constexpr (NP == 2) {
                        tmax = fmaxf(tmax, v);                            // (v >= 0)
                        const _Float16 hi = (_Float16)v, lo = (_Float16)(v - (float)hi);
                        *reinterpret_cast<_Float16*>(AP + off) = hi;
                        *reinterpret_cast<_Float16*>(AP + PL_STRIDE + off) = lo;
                        continue;
                    }
#pragma unroll
                    for (int p = 0; p < 3; ++p) {
                        const unsigned q = s3_pack_rn(v, v);              // both halves = rn(v): the store takes the upper one (ds_write_b16_d16_hi)
                        *reinterpret_cast<uint16_t*>(AP + p * PL_STRIDE + off) = (uint16_t)(q >> 16);
                        if (p < 2) v -= s3_hi(q);
                    }
                }
            __syncthreads();
            f32x16 acc2[2][2];
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j)
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc2[i][j][r] = 0.f;
#pragma unroll
            for (int ks = 0; ks < 8; ++ks) {
                b3load(ks + 1, b3[(ks + 1) & 1]);
                bf16x8 af[2][NP];
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int p = 0; p < NP; ++p) af[i][p] = *(const bf16x8*)(AP + p * PL_STRIDE + ks * KS_STRIDE + i * 1024 + aoff);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int j = 0; j < NJ; ++j) mac6(acc2[i][j], af[i], b3[ks & 1][j], false);
                __builtin_amdgcn_sched_barrier(0);
            }
            if constexpr (NEXT) __syncthreads();              // every wave is past its conv3 reads of AP: the NEXT conv1's operand planes overwrite it
            f32x16 acc1[2];                                 // NEXT: conv1 of the next block, 64 pixels x channels [32 w, 32 w + 32)
            if constexpr (NEXT) {
#pragma unroll
                for (int i = 0; i < 2; ++i) acc1[i] = zero16;
            }
#pragma unroll
            for (int j = 0; j < NJ; ++j) {                    // j = the wave's n-tile: output channels [128 j + 32 w, + 32) (W8: [32 w, + 32)); NEXT: round j = conv1's K half j
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    const int col = (W8 ? w : 4 * j + w) * 32 + (lane & 7) * 4;
                    const f32x4 bv = SKD ? *(const f32x4*)&CB[col] : *(const f32x4*)(a.bias3 + col);
                    f32x4 osc3 = f32x4{1.f, 1.f, 1.f, 1.f};
                    if constexpr (NP == 2) osc3 = SKD ? *(const f32x4*)&CB[256 + col] : *(const f32x4*)(a.oscale3 + col);
                    f32x4 nsc, nsh;
                    if constexpr (NEXT) { const float nxs = s2_xscale(a.n_xscale); nsc = *(const f32x4*)(a.n_scale + col) * nxs; nsh = *(const f32x4*)(a.n_shift + col) * nxs; }
                    int off[4];
                    f32x4 rv[SKD ? 1 : 4], uv[UP ? 4 : 1];
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const int m = 32 * i + (lane >> 3) + 8 * k;
                        const int oy = oy0 + 2 * (m >> 4) + h, ox = ox0 + (m & 15);
                        const bool in = oy < a.OH && ox < a.OW;
                        if constexpr (SKD) off[k] = skoff(4 * h + 2 * j + i, k);           // (the same value)
                        else off[k] = in ? ((oy * a.OW + ox) * a.N2 + col) * 4 : BUF_OOB;
                        if constexpr (!SKD) rv[k] = buf_load(r_srd, off[k], 0);
                        if constexpr (UP && !NEXT) uv[k] = buf_load(up_srd, in ? (((oy >> 1) * (a.OW >> 1) + (ox >> 1)) * a.N2 + col) * 4 : BUF_OOB, 0);
                    }
#pragma unroll
                    for (int r = 0; r < 16; ++r) T[acc_row(r, lane) * 36 + (lane & 31)] = acc2[i][j][r];
                    __builtin_amdgcn_wave_barrier();
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        if constexpr (UP && NEXT) {           // (requested here, one at a time: with the next block's accumulators live there is no room for four)
                            const int m = 32 * i + (lane >> 3) + 8 * k;
                            const int oy = oy0 + 2 * (m >> 4) + h, ox = ox0 + (m & 15);
                            uv[0] = buf_load(up_srd, (oy < a.OH && ox < a.OW) ? (((oy >> 1) * (a.OW >> 1) + (ox >> 1)) * a.N2 + col) * 4 : BUF_OOB, 0);
                        }
                        f32x4 o = *(const f32x4*)&T[((lane >> 3) + 8 * k) * 36 + (lane & 7) * 4];
                        if constexpr (NP == 2) o *= osc3;             // back to scale (an exact power of two per column)
                        if constexpr (SKD) {
                            // The wave's VMEM instructions behind DMA(b, k) that are certain to have been issued by now -- its own DMAs and the blocks' buf_stores, all
                            // unconditional and pinned in this order by the asm statements (hipcc's loads in between only make the wait stricter; vmcnt retires loads and
                            // stores alike in issue order on this target, as hipcc's own counted waits assume):
                            //   block 0 (requested in one go before the pass): DMA(0, k + 1 .. 3), then a pair {DMA(1, q), store(0, q)} for each q < k          = 3 + k
                            //   blocks 1-6: store(b - 1, k), the pairs {DMA(b, q), store(b - 1, q)} for q > k and {DMA(b + 1, q), store(b, q)} for q < k         = 7
                            //   block 7 (requests nothing): store(6, k), the pairs of q > k, store(7, q) for q < k                                             = 7 - k
                            const int b = 4 * h + 2 * j + i;
                            skwait(b == 0 ? 3 + k : b == 7 ? 7 - k : 7);
                            // (a lane outside the map: its slot holds whatever an earlier block's row left there -- the register path's buffer load gives it zero)
                            const f32x4 r = *(const f32x4*)&RB[k * 256 + lane * 4];
                            const bool inmap = off[k] != BUF_OOB;
                            o = (o + bv) + f32x4{inmap ? r[0] : 0.f, inmap ? r[1] : 0.f, inmap ? r[2] : 0.f, inmap ? r[3] : 0.f};
                            if (b < 7) skdma(b + 1, k);               // slot k is free again: the next block's row group, ahead of this block's stores
                        } else {
                            o = (o + bv) + rv[k];
                        }
                        if constexpr (UP) o += uv[NEXT ? 0 : k];
                        buf_store(o, o2_srd, off[k]);
                        if constexpr (NEXT) {
                            // the next block's operand: 2^s_next relu(bn_next(o)) of this pixel's 4 channels (local channel 32 w + 4 (lane & 7) of K half j) as
                            // two fp16 planes in A-operand order -- k-step 2 w + ((lane & 7) >> 2), pixel m, 16-byte half ((lane & 3) >> 1) swapped for pixels 8-15
                            const int m = 32 * i + (lane >> 3) + 8 * k;
                            float xn[4];
#pragma unroll
                            for (int c = 0; c < 4; ++c) xn[c] = fmaxf(fmaf(o[c], nsc[c], nsh[c]), 0.f);
                            tmax = fmaxf(fmaxf(tmax, fmaxf(xn[0], xn[1])), fmaxf(xn[2], xn[3]));
                            unsigned char* d = AP + (2 * w + ((lane & 7) >> 2)) * KS_STRIDE + m * 32 + (((((lane & 3) >> 1) ^ ((m >> 3) & 1))) * 16) + (lane & 1) * 8;
                            split_store4<2, PL_STRIDE>(d, xn[0], xn[1], xn[2], xn[3]);
                        }
                    }
                    __builtin_amdgcn_wave_barrier();
                }
                if constexpr (NEXT) {
                    // K half j of conv1 (channels [128 j, 128 j + 128) = k-steps 8 j .. 8 j + 7, ascending: the order of gemm_bf16x3_kernel): wave w -> n-tile w
                    const __amdgpu_buffer_rsrc_t n1_srd = make_srd(a.n_W1, (size_t)128 * 256 * 2 * sizeof(uint16_t));
                    auto n1load = [&](int q, u32x4 (&b)[2]) {
                        const int ksg = 8 * j + (q < 8 ? q : 7);
#pragma unroll
                        for (int p = 0; p < 2; ++p) b[p] = __builtin_bit_cast(u32x4, buf_load(n1_srd, w3voff + p * 1024, ((ksg * 4 + w) * 2) * 1024));
                    };
                    constexpr int NR = 4;                     // weight k-steps in flight: a k-step is only 6 MFMAs (192 cycles), an L2 round trip three times that
                    u32x4 nb[NR][2];
#pragma unroll
                    for (int q = 0; q < NR - 1; ++q) n1load(q, nb[q]);
                    __syncthreads();                          // the four waves' planes of this K half are complete
#pragma unroll
                    for (int q = 0; q < 8; ++q) {
                        n1load(q + NR - 1, nb[(q + NR - 1) % NR]);
                        bf16x8 af[2][2];
#pragma unroll
                        for (int i = 0; i < 2; ++i)
#pragma unroll
                            for (int p = 0; p < 2; ++p) af[i][p] = *(const bf16x8*)(AP + p * PL_STRIDE + q * KS_STRIDE + i * 1024 + aoff);
                        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                        for (int i = 0; i < 2; ++i) mac6(acc1[i], af[i], nb[q % NR], false);
                        __builtin_amdgcn_sched_barrier(0);
                    }
                    __syncthreads();                          // every wave has read the planes: the next K half / the next pass's conv2 tile may overwrite them
                }
            }
            if constexpr (NEXT) {
                // conv1's epilogue as gemm_bf16x3_kernel's: acc * oscale + bias, ReLU, 16-byte stores of the wave's 32 channels of the 64 pixels
                const int col = w * 32 + (lane & 7) * 4;
                const f32x4 b1 = *(const f32x4*)(a.n_b1 + col), o1 = *(const f32x4*)(a.n_osc1 + col);
                const size_t cropn = (size_t)a.OH * a.OW * 128;
                const __amdgpu_buffer_rsrc_t n_srd = make_srd(a.n_out + (size_t)l * cropn, cropn * sizeof(float));
#pragma unroll
                for (int i = 0; i < 2; ++i) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) T[acc_row(r, lane) * 36 + (lane & 31)] = acc1[i][r];
                    __builtin_amdgcn_wave_barrier();
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const int m = 32 * i + (lane >> 3) + 8 * k;
                        const int oy = oy0 + 2 * (m >> 4) + h, ox = ox0 + (m & 15);
                        f32x4 o = *(const f32x4*)&T[((lane >> 3) + 8 * k) * 36 + (lane & 7) * 4];
                        o *= o1;
                        o += b1;
#pragma unroll
                        for (int c = 0; c < 4; ++c) o[c] = fmaxf(o[c], 0.f);
                        buf_store(o, n_srd, (oy < a.OH && ox < a.OW) ? ((oy * a.OW + ox) * 128 + col) * 4 : BUF_OOB);
                    }
                    __builtin_amdgcn_wave_barrier();
                }
            }
            if (h == 0 && !NEXT) __syncthreads();             // every wave is done with the A planes of pass 0 (NEXT: the K half's closing barrier)
        }
        if constexpr (NP == 2) s2_raise(a.range_flag, tmax);
        return;
    }

    if constexpr (FUSE && !TX3) {
        // ---- tail of the Residual block (layers/Residual.py:27-35) exactly as in csrc/conv_wino.hip: conv3 (1x1, 128 -> 256) + bias + skip
        // on relu(conv2 + bias2), on the fp32 pipe: the conv2 tile goes through LDS (pitch 132) as the A operand, 2 x 4 accumulators
        constexpr int MP = 132;
        static_assert(128 * MP <= 2 * HSZ + VFLOATS, "the conv2 tile must fit the workgroup's LDS");
        float* M2 = &S[0];
        const int wm = w >> 1, wn = w & 1;
        const int NB2 = a.N2 >> 5;
        const __amdgpu_buffer_rsrc_t w3_srd = make_srd(a.W3p, (size_t)a.N * a.N2 * sizeof(float));
        const size_t crop2 = (size_t)a.OH * a.OW * a.N2;
        const __amdgpu_buffer_rsrc_t r_srd = make_srd(a.R + (size_t)l * crop2, crop2 * sizeof(float));
        const __amdgpu_buffer_rsrc_t o2_srd = make_srd(a.out2 + (size_t)l * crop2, crop2 * sizeof(float));
        constexpr bool has_up = UP;
        const __amdgpu_buffer_rsrc_t up_srd = make_srd(has_up ? a.up + (size_t)l * (crop2 / 4) : a.R, has_up ? crop2 / 4 * sizeof(float) : 0);
        const float b2v = a.bias[w * 32 + (lane & 31)];
        const int w3voff = lane * 16;
        auto b3load = [&](int q, f32x4(&b)[4]) {
            const int kg = q < 16 ? q : 15;
#pragma unroll
            for (int j = 0; j < 4; ++j) b[j] = buf_load(w3_srd, w3voff, (kg * NB2 + wn * 4 + j) * 1024);
        };
        constexpr int R3 = 3;
        f32x4 b3[R3][4];
#pragma unroll
        for (int r = 0; r < R3 - 1; ++r) b3load(r, b3[r]);
#pragma unroll
        for (int p = 0; p < 4; ++p)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int t = acc_row(r, lane);
                const int pix = (2 * (t >> 3) + (p >> 1)) * X_TW + 2 * (t & 7) + (p & 1);
                M2[pix * MP + w * 32 + (lane & 31)] = fmaxf(out[p][r] + b2v, 0.f);
            }
        __syncthreads();
        f32x16 acc2[2][4];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc2[i][j][r] = 0.f;
        const float* ms = M2 + ((wm * 2) * 32 + (lane & 31)) * MP + (lane >> 5) * 4;
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            b3load(q + R3 - 1, b3[(q + R3 - 1) % R3]);
            __builtin_amdgcn_sched_barrier(0);
            f32x4 af[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) af[i] = *(const f32x4*)(ms + i * 32 * MP + q * 8);
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j) acc2[i][j] = mfma32(af[i][t], b3[q % R3][j][t], acc2[i][j]);
            __builtin_amdgcn_sched_barrier(0);
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float* T = M2 + w * (32 * 36);
                const int col = (wn * 4 + j) * 32 + (lane & 7) * 4;
                const f32x4 bv = *(const f32x4*)(a.bias3 + col);
                int off[4];
                f32x4 rv[4], uv[UP ? 4 : 1];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int pp = (wm * 2 + i) * 32 + (lane >> 3) + 8 * k;
                    const int oy = oy0 + pp / X_TW, ox = ox0 + pp % X_TW;
                    const bool in = oy < a.OH && ox < a.OW;
                    off[k] = in ? ((oy * a.OW + ox) * a.N2 + col) * 4 : BUF_OOB;
                    rv[k] = buf_load(r_srd, off[k], 0);
                    if constexpr (UP) uv[k] = buf_load(up_srd, in ? (((oy >> 1) * (a.OW >> 1) + (ox >> 1)) * a.N2 + col) * 4 : BUF_OOB, 0);
                }
#pragma unroll
                for (int r = 0; r < 16; ++r) T[acc_row(r, lane) * 36 + (lane & 31)] = acc2[i][j][r];
                __builtin_amdgcn_wave_barrier();
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    f32x4 o = (*(const f32x4*)&T[((lane >> 3) + 8 * k) * 36 + (lane & 7) * 4] + bv) + rv[k];
                    if constexpr (UP) o += uv[k];
                    buf_store(o, o2_srd, off[k]);
                }
                __builtin_amdgcn_wave_barrier();
            }
        return;
    }

    if constexpr (NT == 2 || W8) {
        // the two component halves of an n-tile meet (W8: they already have, above).  Wave wc = 0 holds rows xi = 0, 1 (out[0..1] = R of row 0, out[2..3] = R of row 1), wave wc = 1
        // rows xi = 2, 3 (row 3 negated in the weights).  Y[0][j] = R0 + R1 + R2, Y[1][j] = R1 - R2 + R3': wave wc keeps output row i = wc and
        // hands its MIDDLE row (1 or 2) to the partner through LDS ([position][register][lane]: conflict-free).
        if constexpr (NT == 2) {
            float* X = &S[2 * HSZ];                            // (the last chunk's closing barrier has passed: V is free)
#pragma unroll
            for (int q = 0; q < 2; ++q)
#pragma unroll
                for (int r = 0; r < 16; ++r) X[((w * 2 + q) * 16 + r) * 64 + lane] = wc == 0 ? out[2 + q][r] : out[q][r];
            __syncthreads();
            const int pw = (1 - wc) * 2 + wn;
#pragma unroll
            for (int q = 0; q < 2; ++q)
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    mine[q][r] = (wc == 0 ? out[q][r] + out[2 + q][r] : out[2 + q][r] - out[q][r]) + X[((pw * 2 + q) * 16 + r) * 64 + lane];
            __syncthreads();                                  // the exchange area becomes the transposition patches
        }
        float* T = &S[2 * HSZ] + w * (32 * 36);
        const int col = wn * 32 + (lane & 7) * 4;
        const f32x4 bv = *(const f32x4*)(a.bias + col);
        f32x4 osc = f32x4{1.f, 1.f, 1.f, 1.f};
        if constexpr (NP == 2) osc = *(const f32x4*)(a.oscale + col);
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int p = 2 * wc + q, pi = p >> 1, pj = p & 1;
#pragma unroll
            for (int r = 0; r < 16; ++r) T[acc_row(r, lane) * 36 + (lane & 31)] = mine[q][r];
            __builtin_amdgcn_wave_barrier();
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int t = (lane >> 3) + 8 * k;
                const int oy = oy0 + 2 * (t >> 3) + pi, ox = ox0 + 2 * (t & 7) + pj;
                f32x4 o = *(const f32x4*)&T[t * 36 + (lane & 7) * 4];
                if constexpr (NP == 2) o *= osc;
                o += bv;
                if (a.relu) {
#pragma unroll
                    for (int z = 0; z < 4; ++z) o[z] = fmaxf(o[z], 0.f);
                }
                buf_store(o, out_srd, (oy < a.OH && ox < a.OW) ? ((oy * a.OW + ox) * a.N + col) * 4 : BUF_OOB);
            }
            __builtin_amdgcn_wave_barrier();
        }
        return;
    }

    // ---- epilogue (plain convolution): per output position transpose the 32 tiles x 32 channels through a wave-private patch -> 16-byte stores
    float* T = &S[2 * HSZ] + w * (32 * 36);
    const int col = w * 32 + (lane & 7) * 4;
    const f32x4 bv = *(const f32x4*)(a.bias + col);
    f32x4 osc = f32x4{1.f, 1.f, 1.f, 1.f};
    if constexpr (NP == 2) osc = *(const f32x4*)(a.oscale + col);
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const int pi = p >> 1, pj = p & 1;
#pragma unroll
        for (int r = 0; r < 16; ++r) T[acc_row(r, lane) * 36 + (lane & 31)] = out[p][r];
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int t = (lane >> 3) + 8 * k;
            const int oy = oy0 + 2 * (t >> 3) + pi, ox = ox0 + 2 * (t & 7) + pj;
            f32x4 o = *(const f32x4*)&T[t * 36 + (lane & 7) * 4];
            if constexpr (NP == 2) o *= osc;
            o += bv;
            if (a.relu) {
#pragma unroll
                for (int q = 0; q < 4; ++q) o[q] = fmaxf(o[q], 0.f);
            }
            buf_store(o, out_srd, (oy < a.OH && ox < a.OW) ? ((oy * a.OW + ox) * a.N + col) * 4 : BUF_OOB);
        }
        __builtin_amdgcn_wave_barrier();
    }
