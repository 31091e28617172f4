// scan_ls.hip -- selective SSM scan, forward and backward, "lanes = states" kernels (gfx950, wave64).
//
// Same math as the reference kernels (selective_scan_fwd_kernel.cuh:67-303, selective_scan_bwd_kernel.cuh:75-489,
// real A, variable B / C); the mapping is built on what tools/valu_lab*.hip measured on MI355X:
// a VGPR-only v_fma / v_mul / v_add issues at 32 lanes per clock, a v_exp_f32 costs ~3.5 of them, and every
// cross-lane form (DPP, v_readlane, v_permlane*_swap) and every SGPR-operand form issues at half rate or worse.
// So the recurrences must be serial IN a lane, and the operands a lane cannot own must cost one DPP each, no more.
//
//   * a 16-lane ROW is one (batch, channel) stream; the lane index inside the row is the STATE n, so the 16 (32, 64)
//     recurrences h_n <- a_n h_n + b_n of a channel run side by side, one per lane, serial along the tokens: no
//     scan, no carry between lanes, no barrier.  dstate 32 / 64 take 2 / 4 rows per channel.
//   * a TILE is 16 tokens.  What is shared by the states of a channel -- delta_t, delta_t u_t, dy_t -- is computed once,
//     by the lane that holds token t of the tile (lane r holds token bitrev4(r), see below), and enters the
//     recurrence of all 16 lanes as a DPP row broadcast operand (v_mul_f32_dpp ... row_newbcast).  What differs per
//     state -- B_{n,t}, C_{n,t}, A_n -- is the lane's own: it loads 16 consecutive tokens of ITS row of B and C.
//   * sums over the states (y_t; S1_t = sum_n g B, S2_t = sum_n A g a h) are transposed 16 x 16 reductions: pairs of
//     token-vectors are merged with two masked DPP adds per level (bank_mask for the 8- and 4-lane levels, a select
//     pair for the 2- and 1-lane ones), 30 DPP adds for 16 tokens, and leave the total of token t in the lane that owns
//     token t -- the bit-reversed token order is what makes the merge tree consume tokens in loop order.
//   * backward: the forward states of a tile are recomputed from the forward kernel's checkpoint (one row of `x`
//     per 16 * rows tokens: 4 bytes per token and channel, written by the forward kernels of this file and by
//     scan_fwd_chan.hip) and kept in registers (a_t, h_t: 32 VGPRs) for the reverse sweep over the same 16 tokens.
//   * dB_{n,t} / dC_{n,t} are sums over channels: a row walks kLsCPR channels per tile and keeps the sum in
//     registers; the rows and waves of a workgroup (16 * W channels of one B/C group) are then added through LDS in
//     fixed order.  When the workgroup covers its whole group (Vivim stage 0: 128 channels) the result is STORED:
//     no atomics, bit-reproducible; wider groups add one fp32 atomic per workgroup (reference: one per channel,
//     selective_scan_bwd_kernel.cuh:312-313).
//   * the token axis is cut into segments for parallelism (scan_plan.hip: ls_segmentation); a segment's inflow (h from the left in
//     the forward, g from the right in the backward) comes from a pre-pass (recurrence only) and a carry kernel.
// No alignment requirement: every activation access is one element per lane.
#include "scan_plan.cuh"

namespace vivim {


// =========================================================================================================================
// Backward, main kernel.  One loop over (tile, channel) steps, tiles right to left, the row's kLsCPR channels inside a
// tile.  What a channel carries from tile to tile (the reverse carry, dA, dD, dbias partial sums) lives in wave-private
// LDS, 4 floats per lane and channel, so the loop body holds ONE channel's registers and is not unrolled over channels
// (the unrolled first version: 4 x the code, its scalar state spilled to VGPR lanes).  The activations of step i + 1 are
// requested before step i is computed.
// =========================================================================================================================
// DET (vivim_selective_scan_bwd_det): dA / dD / dbias are stored into the (batch, segment) slot of the workspace p points
// them at.  dB / dC keep their adds while a group has at most two workgroups (0 + a + b == 0 + b + a exactly); with
// more, p's dB / dC point into the workspace too and the workgroup's index within its group is the slot.
template <typename T, int NS, bool HAS_Z, bool DET = false>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(NS == 16 ? 3 : 2, 3))) ssm_ls_bwd_kernel(const vivim_ssm_bwd_params p, const LsSeg sg) {
    typedef LsGeom<NS> G;
    constexpr int RPS = G::RPS, SPW = G::SPW, CPW = G::CPW, CPR = kLsCPR;
    const vivim_ssm_fwd_params& f = p.f;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), W = blockDim.x >> 6;
    const int row = lane >> 4, li = lane & 15;
    const int rs = row % RPS, sw = row / RPS;
    const int n = rs * 16 + li;                               // this lane's state
    const int tk = ((li & 1) << 3) | ((li & 2) << 1) | ((li & 4) >> 1) | ((li & 8) >> 3);   // this lane's token of a tile
    const int b = blockIdx.y, seg = blockIdx.z;
    const int L = ls_own(f.seqlen), cpg = f.dim / f.n_groups;
    const int cpb = W * CPW;                                  // channels per workgroup
    const int bpg = (cpg + cpb - 1) / cpb;                    // workgroups per B/C group
    const int g = blockIdx.x / bpg;
    const int d_end = ls_own((g + 1) * cpg);
    const int dwave = ls_own(g * cpg + (blockIdx.x - g * bpg) * cpb + wave * CPW);     // first channel of this wave (uniform)
    const int rowch = sw * CPR;                               // this row's first channel, relative to the wave's
    const int ntiles = (L + kLsT - 1) / kLsT;
    const int nck = (ntiles + RPS - 1) / RPS;                 // checkpoint rows of x
    const int blk_lo = seg * sg.seg_blocks, blk_hi = min(nck, blk_lo + sg.seg_blocks);
    const int tile_lo = blk_lo * RPS, tile_hi = min(ntiles, blk_hi * RPS);
    const int t_next = blk_hi * G::CK;                        // first token right of the segment
    const bool single = ls_own((int)(bpg == 1)) != 0;         // this workgroup is the only contributor to its dB / dC rows

    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* slot = smem + ((wave * SPW + sw) * 2 * NS + n) * 16;          // [wave][stream][dB | dC][n][16 tokens]
    constexpr int NF = 4 + RPS - 1;                           // per-lane fields per channel (+ inner block boundaries, dstate 32 / 64)
    float* cstate = smem + W * SPW * 2 * NS * 16 + wave * (CPR * NF * kWave) + lane;   // [wave][channel][field][lane]
    // carried: GCAR, DACC, DDACC, DBIAS.  D and delta_bias are per channel only: a small table [wave][channel][row][D | bias]
    // behind the per-lane fields; A * log2e of the row's channels stays in registers (3 workgroups per CU: <= 53 KB each)
    enum { GCAR = 0, DACC = 1, DDACC = 2, DBIAS = 3, HSUB = 4 };
    float* ctab = smem + W * SPW * 2 * NS * 16 + W * (CPR * NF * kWave) + (wave * CPR * 4 + row) * 2;
    // B / C rows of the NEXT tile, raw: [B | C][state][16 tokens]; filled by the whole workgroup between the two barriers of
    // a tile's epilogue (the loads are issued a step earlier), read by every wave at the top of the next tile
    unsigned char* stage = reinterpret_cast<unsigned char*>(smem + W * SPW * 2 * NS * 16 + W * (CPR * NF * kWave) + W * CPR * 8);
    constexpr int PT = NS * (int)sizeof(T);                   // 16-byte pieces per tensor and tile
    static_assert(CPR == 4, "the per-channel A registers are selected by hand");

    typedef vivim_ssm_bwd_params BP;
    LsTensorR<T> tu, tdl, tdo;                                // loaded first in every step: resident
    LsTensor<T> tz, to, tdu, tdd, tdz, toz;                   // the rest: through the kernel arguments
    tu.init(f.u, b * f.u_batch_stride, f.u_d_stride, rowch);
    tdl.init(f.delta, b * f.delta_batch_stride, f.delta_d_stride, rowch);
    tdo.init(p.dout, b * p.dout_batch_stride, p.dout_d_stride, rowch);
    tdu.init(LS_OFF(BP, du), LS_OFF(BP, du_batch_stride), b, p.du_d_stride, rowch);
    tdd.init(LS_OFF(BP, ddelta), LS_OFF(BP, ddelta_batch_stride), b, p.ddelta_d_stride, rowch);
    if (HAS_Z) {
        tz.init(LS_OFF(BP, f.z), LS_OFF(BP, f.z_batch_stride), b, f.z_d_stride, rowch);
        to.init(LS_OFF(BP, f.out), LS_OFF(BP, f.out_batch_stride), b, f.out_d_stride, rowch);
        tdz.init(LS_OFF(BP, dz), LS_OFF(BP, dz_batch_stride), b, p.dz_d_stride, rowch);
        toz.init(LS_OFF(BP, f.out_z), LS_OFF(BP, f.out_z_batch_stride), b, f.out_z_d_stride, rowch);
    }
    LsCkpt tx;
    tx.init(LS_OFF(BP, f.x), b, f.dim, nck, NS, rowch);
    LsRow<T> rB, rC;
    rB.init(LS_OFF(BP, f.B), LS_OFF(BP, f.B_batch_stride), b, g, f.B_dstate_stride, n);
    rC.init(LS_OFF(BP, f.C), LS_OFF(BP, f.C_batch_stride), b, g, f.C_dstate_stride, n);
    float* __restrict__ dBg = ls_own(static_cast<float*>(p.dB) + b * p.dB_batch_stride + g * p.dB_group_stride);
    float* __restrict__ dCg = ls_own(static_cast<float*>(p.dC) + b * p.dC_batch_stride + g * p.dC_group_stride);
    const int dBns = ls_own((int)p.dB_dstate_stride), dCns = ls_own((int)p.dC_dstate_stride);
    const bool softplus = ls_own((int)f.delta_softplus) != 0, want_oz = HAS_Z && ls_own((int)(f.out_z != nullptr)) != 0;
    const bool bc_vec = ls_own(sg.bc_vec) != 0;

    // ---- per-channel state: the reverse carry a_{t+1} g_{t+1} of the token that is processed next, and three sums ----
    float A2r[CPR];
#pragma unroll
    for (int c = 0; c < CPR; ++c) {
        const int d = dwave + rowch + c;
        const bool cv = d < d_end;
        const int dc = cv ? d : d_end - 1;
        const float A2 = static_cast<const float*>(f.A)[dc * f.A_d_stride + n * f.A_dstate_stride] * kLog2e;
        const float bias = f.delta_bias ? static_cast<const float*>(f.delta_bias)[dc] : 0.0f;
        const float gin = (sg.S > 1 && cv) ? sg.gin[(((int64_t)b * f.dim + dc) * sg.S + seg) * NS + n] : 0.0f;
        float dl_nx = 0.0f;                                   // delta of the first token right of the segment
        if (t_next < L) {
            const float raw = tdl.ld(min(dwave + c, d_end - 1), t_next, cv) + bias;
            dl_nx = softplus ? softplus_ref(raw) : raw;
        }
        float* cs = cstate + c * NF * kWave;
        cs[GCAR * kWave] = gin * fast_exp2(dl_nx * A2);
        cs[DACC * kWave] = 0.0f; cs[DDACC * kWave] = 0.0f; cs[DBIAS * kWave] = 0.0f;
        A2r[c] = A2;
        ctab[c * 8 + 0] = f.D ? static_cast<const float*>(f.D)[dc] : 0.0f;      // every lane of the row writes the same value
        ctab[c * 8 + 1] = bias;
    }

    // what a step reads from memory for this lane: requested one step ahead
    struct Raw { float uu, raw, dy, zf, of, hin; };
    auto fetch = [&](int tile, int c) __attribute__((always_inline)) -> Raw {
        Raw r;
        const ls_kargs q = ls_fresh_kargs();
        const int t = tile * kLsT + tk;
        const int d = dwave + rowch + c;
        const bool cv = d < d_end;
        const int chu = min(dwave + c, d_end - 1);
        const bool ok = cv && t < L && tile >= tile_lo;   // past the segment's last step: nothing is used
        r.uu = tu.ld_raw(chu, t, ok);
        r.raw = tdl.ld_raw(chu, t, ok);
        r.dy = tdo.ld_raw(chu, t, ok);
        r.zf = 0.0f; r.of = 0.0f;
        if (HAS_Z) { r.zf = tz.ld_raw(q, chu, t, ok); r.of = to.ld_raw(q, chu, t, ok); }
        const int blk = tile / RPS;
        r.hin = tx.ld_raw(q, chu, (blk - 1) * NS + n, blk > 0 && cv && tile >= tile_lo);
        return r;
    };

    float Bv[16], Cv[16], dBv[16], dCv[16];
    bool staged = false;
    Raw nxt = fetch(tile_hi - 1, 0);
    // The per-token outputs of a step are stored at the START of the next one, between the first use of that step's inputs
    // and the request for the inputs of the one after: a step's loads then have a whole step to land, and the wait in
    // front of the first use (hipcc writes vmcnt(0) there, it cannot count across the loop edge) only meets stores that
    // were issued a step earlier.
    float p_du = 0.0f, p_dd = 0.0f, p_dz = 0.0f, p_oz = 0.0f;
    int p_chu = min(dwave, d_end - 1), p_t = 0;
    bool p_st = false;
    auto flush = [&]() __attribute__((always_inline)) {
        const ls_kargs qs = ls_fresh_kargs();
        if (HAS_Z) {
            tdz.st(qs, p_chu, p_t, p_st, p_dz);
            if (want_oz) toz.st(qs, p_chu, p_t, p_st, p_oz);
        }
        tdu.st(qs, p_chu, p_t, p_st, p_du);
        tdd.st(qs, p_chu, p_t, p_st, p_dd);
    };
#pragma unroll 1
    for (int tile = tile_hi - 1; tile >= tile_lo; --tile) {
        const int t0 = tile * kLsT;
        const int t = t0 + tk;
        const bool tv = t < L;
        const int blk = tile / RPS, j = tile - blk * RPS;
        if (staged) {                                         // this tile's rows were staged during the previous one
            constexpr int NV = (int)sizeof(T);
            u32x4 rb[NV], rc[NV];
#pragma unroll
            for (int i = 0; i < NV; ++i) {
                rb[i] = *reinterpret_cast<const u32x4*>(stage + (n * NV + i) * 16);
                rc[i] = *reinterpret_cast<const u32x4*>(stage + (PT + n * NV + i) * 16);
            }
            LsUnpack<T>::run(rb, Bv);
            LsUnpack<T>::run(rc, Cv);
        } else {
            const bool vec = bc_vec && t0 + kLsT <= L;
            const ls_kargs q = ls_fresh_kargs();
            rB.load16(q, t0, L, vec, Bv);
            rC.load16(q, t0, L, vec, Cv);
        }
#pragma unroll
        for (int k = 0; k < 16; ++k) { dBv[k] = 0.0f; dCv[k] = 0.0f; }
        ls_arrive(Bv);
        ls_arrive(Cv);
        const bool stage_next = W == 4 && bc_vec && tile - 1 >= tile_lo;   // (a tile left of another one is whole)
        u32x4 sb = {0u, 0u, 0u, 0u}, sc = {0u, 0u, 0u, 0u};
#pragma unroll 1
        for (int c = 0; c < CPR; ++c) {
            Raw cur = nxt;                                    // as loaded: lanes that are off hold the element at offset 0
            const int d = dwave + rowch + c;
            const bool cv = d < d_end;                        // uniform per row
            const int chu = min(dwave + c, d_end - 1);        // uniform part of the channel, clamped to a valid one
            const bool ok = cv && tv;
            cur.uu = ok ? cur.uu : 0.0f; cur.raw = ok ? cur.raw : 0.0f; cur.dy = ok ? cur.dy : 0.0f;
            if (HAS_Z) { cur.zf = ok ? cur.zf : 0.0f; cur.of = ok ? cur.of : 0.0f; }
            cur.hin = (cv && blk > 0) ? cur.hin : 0.0f;
            {   // "used here": the selects must not drift below the next step's loads
                float u0 = cur.uu, u1 = cur.raw, u2 = cur.dy, u3 = cur.zf, u4 = cur.of, u5 = cur.hin;
                asm volatile("" : "+v"(u0), "+v"(u1), "+v"(u2), "+v"(u3), "+v"(u4), "+v"(u5));
                cur.uu = u0; cur.raw = u1; cur.dy = u2; cur.zf = u3; cur.of = u4; cur.hin = u5;
            }
            flush();                                          // the previous step's outputs
            nxt = fetch(c + 1 < CPR ? tile : tile - 1, c + 1 < CPR ? c + 1 : 0);
            if (c == CPR - 1 && stage_next) {                 // the next tile's B / C rows: one 16-byte piece of each per thread
                const ls_kargs q = ls_fresh_kargs();
                const bool mine = tid < PT;
                const unsigned pn = (unsigned)tid / (unsigned)sizeof(T), pp = (unsigned)tid % (unsigned)sizeof(T);
                sb = rB.piece(q, (tile - 1) * kLsT, mine ? pn : 0u, mine ? pp : 0u);
                sc = rC.piece(q, (tile - 1) * kLsT, mine ? pn : 0u, mine ? pp : 0u);
            }
            const bool st = ok && rs == 0;                    // one row of a stream stores the per-token outputs
            float* cs = cstate + c * NF * kWave;
            // ---- this lane's token of channel d ----
            float dy = cur.dy;
            if (HAS_Z) {
                const float sgm = sigmoidf_fast(cur.zf);
                const float dzv = dy * cur.of * sgm * (1.0f + cur.zf * (1.0f - sgm));        // bwd_kernel.cuh:186-191
                dy *= cur.zf * sgm;
                p_dz = dzv;
                p_oz = cur.of * cur.zf * sgm;                                                 // bwd_kernel.cuh:193-204
            }
            const float raw = cur.raw + ctab[c * 8 + 1];
            float dl = ok ? (softplus ? softplus_ref(raw) : raw) : 0.0f;                     // padded tokens: identity step
            float w = dl * cur.uu;
            cs[DDACC * kWave] += dy * cur.uu;
            ls_settle(dl, w, dy);
            const float A2 = c == 0 ? A2r[0] : c == 1 ? A2r[1] : c == 2 ? A2r[2] : A2r[3];
            // ---- forward states of the tile, from the checkpoint (dstate 32 / 64: from the block's inner boundaries) ----
            float h_in = cur.hin;
            if constexpr (RPS > 1) {
                if (tile == min(tile_hi, (blk + 1) * RPS) - 1) {  // first tile of this block to be processed: rebuild the
                    float h = cur.hin;                             // states at the block's inner tile boundaries
                    const float bias = ctab[c * 8 + 1];
                    const ls_kargs qs = ls_fresh_kargs();
                    for (int jj = 0; jj < j; ++jj) {
                        const int t0j = (blk * RPS + jj) * kLsT, tj = t0j + tk;
                        const bool okj = cv && tj < L;
                        float Bj[16];
                        rB.load16(qs, t0j, L, bc_vec && t0j + kLsT <= L, Bj);
                        const float uj = tu.ld(chu, tj, okj);
                        const float rawj = tdl.ld(chu, tj, okj) + bias;
                        float dlj = okj ? (softplus ? softplus_ref(rawj) : rawj) : 0.0f;
                        float wj = dlj * uj;
                        ls_settle(dlj, wj);
                        sfor<0, 16>([&](auto kc) {
                            constexpr int k = decltype(kc)::value;
                            const float a = fast_exp2(tok<k>(dlj) * A2);
                            h = tok_fma<k>(a * h, wj, Bj[k]);
                        });
                        cs[(HSUB + jj) * kWave] = h;          // kept per channel until the block's first tile is done
                    }
                }
                if (j > 0) h_in = cs[(HSUB + j - 1) * kWave];
            }
            float a[16], h[16];
            {
                float hp = h_in;
                sfor<0, 16>([&](auto kc) {
                    constexpr int k = decltype(kc)::value;
                    a[k] = fast_exp2(tok<k>(dl) * A2);
                    hp = tok_fma<k>(a[k] * hp, w, Bv[k]);                                  // h_t = a_t h_{t-1} + d_t u_t B_t
                    h[k] = hp;
                });
            }
            // ---- reverse sweep: g_t = a_{t+1} g_{t+1} + C_t dy_t; ag = a_t g_t is the carry to the left ----
            float s1[16], s2[16], z1[8], z2[8], w1[4], w2[4], v1[2], v2[2], S1, S2;
            {
                float ag = cs[GCAR * kWave], dA0 = cs[DACC * kWave], dA1 = 0.0f;
                sfor_down<16>([&](auto kc) {
                    constexpr int k = decltype(kc)::value;
                    const float gk = tok_fma<k>(ag, dy, Cv[k]);                          // g_t
                    ag = gk * a[k];
                    const float x = ag * (k > 0 ? h[k > 0 ? k - 1 : 0] : h_in);          // g_t a_t h_{t-1}
                    s1[k] = gk * Bv[k];
                    s2[k] = A2 * x;
                    if constexpr (k & 1) dA1 = tok_fma<k>(dA1, dl, x); else dA0 = tok_fma<k>(dA0, dl, x);   // two chains
                    dBv[k] = tok_fma<k>(dBv[k], w, gk);
                    dCv[k] = tok_fma<k>(dCv[k], dy, h[k]);
                    ls_reduce_down<k>(s1, z1, w1, v1, S1, li);
                    ls_reduce_down<k>(s2, z2, w2, v2, S2, li);
                });
                cs[GCAR * kWave] = ag;
                cs[DACC * kWave] = dA0 + dA1;
            }
            S1 = ls_rows_sum<RPS>(S1);
            S2 = ls_rows_sum<RPS>(S2);
            // ---- per-token outputs (this lane's token) ----
            const float duv = fmaf(dl, S1, ctab[c * 8 + 0] * dy);
            float ddv = fmaf(cur.uu, S1, S2 * kLn2);                                      // S2 carries A * log2e
            if (softplus && raw <= 20.0f) ddv *= sigmoidf_fast(raw);                      // bwd_kernel.cuh:439-452
            cs[DBIAS * kWave] += ok ? ddv : 0.0f;
            p_du = duv; p_dd = ddv; p_chu = chu; p_t = t; p_st = st;
        }
        // ---- dB / dC of the tile: this row's channels are summed; add the rows and waves of the workgroup ----
        // Both barriers sit around the slot writes: the first says "everybody is done reading the previous tile's slots and
        // this tile's staged rows", the second "slots and the next tile's rows are written".  Back to back, the second
        // finds the waves already aligned; spaced (one before, one after the reduction) they cost two synchronisations.
        lds_barrier();
        if (stage_next && tid < PT) {
            *reinterpret_cast<u32x4*>(stage + tid * 16) = sb;
            *reinterpret_cast<u32x4*>(stage + (PT + tid) * 16) = sc;
        }
        staged = stage_next;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            *reinterpret_cast<float4*>(slot + q * 4) = float4{dBv[q * 4], dBv[q * 4 + 1], dBv[q * 4 + 2], dBv[q * 4 + 3]};
            *reinterpret_cast<float4*>(slot + NS * 16 + q * 4) = float4{dCv[q * 4], dCv[q * 4 + 1], dCv[q * 4 + 2], dCv[q * 4 + 3]};
        }
        lds_barrier();
        {
            const int nsrc = W * SPW;
            for (int e = tid; e < 2 * NS * 16; e += blockDim.x) {
                const float* sp = smem + e;
                float acc = sp[0];
                for (int s = 1; s < nsrc; ++s) acc += sp[s * 2 * NS * 16];
                const int isC = e / (NS * 16), en = (e / 16) % NS, ek = e & 15;
                if (t0 + ek < L) {
                    float* dst = isC ? dCg + en * dCns : dBg + en * dBns;
                    if (single) dst[t0 + ek] = acc;                   // the only contributor: plain store, deterministic
                    else if (DET && bpg > 2) dst[(int64_t)(blockIdx.x - g * bpg) * f.batch * f.n_groups * NS * L + t0 + ek] = acc;
                    else atomicAdd(dst + t0 + ek, acc);               // two workgroups: still order-independent (a + b)
                }
            }
        }
    }
    flush();
    // ---- per-channel sums ----
    for (int c = 0; c < CPR; ++c) {
        const int d = dwave + rowch + c;
        const float* cs = cstate + c * NF * kWave;
        const float sD = ls_row_total(cs[DDACC * kWave]), sb = ls_row_total(cs[DBIAS * kWave]);
        if (d >= d_end) continue;                             // uniform per row
        const int64_t dslot = DET ? (int64_t)(b * gridDim.z + seg) * f.dim : 0;
        det_add<DET>(static_cast<float*>(p.dA) + dslot * NS + d * p.dA_d_stride + n * p.dA_dstate_stride, cs[DACC * kWave]);
        if (li == 0 && rs == 0) {
            if (p.dD) det_add<DET>(static_cast<float*>(p.dD) + dslot + d, sD);
            if (p.ddelta_bias) det_add<DET>(static_cast<float*>(p.ddelta_bias) + dslot + d, sb);
        }
    }
}

// =========================================================================================================================
// Backward, pre-pass of the token-axis split: per (batch, channel, segment >= 1, state)
//   agg  = g at the segment's first token for zero inflow from the right
//   dsum = sum over the segment of delta_{t+1}
// ONE channel per row here (a wave = 4 / RPS channels): four times the waves of the main kernel for the same cut -- the
// recurrence is all there is, so what has to be hidden is load latency -- and nothing carried per channel but three
// registers.  The next tile's inputs are requested before the current tile is computed.  No LDS, no barrier.
// =========================================================================================================================
template <typename T, int NS, bool HAS_Z>
__global__ void __launch_bounds__(256) ssm_ls_bwd_prepass_kernel(const vivim_ssm_bwd_params p, const LsSeg sg) {
    typedef LsGeom<NS> G;
    constexpr int RPS = G::RPS, SPW = G::SPW;
    const vivim_ssm_fwd_params& f = p.f;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), W = blockDim.x >> 6;
    const int row = lane >> 4, li = lane & 15;
    const int rs = row % RPS, sw = row / RPS;
    const int n = rs * 16 + li;
    const int tk = ((li & 1) << 3) | ((li & 2) << 1) | ((li & 4) >> 1) | ((li & 8) >> 3);
    const int b = blockIdx.y, seg = blockIdx.z + 1;           // segment 0 has no left neighbour to feed
    const int L = f.seqlen, cpg = f.dim / f.n_groups;
    const int cpb = W * SPW;                                  // channels per workgroup
    const int bpg = (cpg + cpb - 1) / cpb;
    const int g = blockIdx.x / bpg;
    const int d_end = (g + 1) * cpg;
    const int dwave = g * cpg + (blockIdx.x - g * bpg) * cpb + wave * SPW;    // first channel of this wave (uniform)
    if (dwave >= d_end) return;                               // whole waves only
    const int d = dwave + sw;                                 // this row's channel
    const bool cv = d < d_end;
    const int dc = cv ? d : d_end - 1;
    const int ntiles = (L + kLsT - 1) / kLsT;
    const int nck = (ntiles + RPS - 1) / RPS;
    const int blk_lo = seg * sg.seg_blocks, blk_hi = min(nck, blk_lo + sg.seg_blocks);
    const int tile_lo = blk_lo * RPS, tile_hi = min(ntiles, blk_hi * RPS);
    const int t_first = blk_lo * G::CK, t_next = blk_hi * G::CK;
    typedef vivim_ssm_bwd_params BP;
    LsTensorR<T> tdl, tdo, tz;
    tdl.init(f.delta, b * f.delta_batch_stride, f.delta_d_stride, sw);
    tdo.init(p.dout, b * p.dout_batch_stride, p.dout_d_stride, sw);
    if (HAS_Z) tz.init(f.z, b * f.z_batch_stride, f.z_d_stride, sw);
    LsRow<T> rC;
    rC.init(LS_OFF(BP, f.C), LS_OFF(BP, f.C_batch_stride), b, g, f.C_dstate_stride, n);
    const float A2 = static_cast<const float*>(f.A)[dc * f.A_d_stride + n * f.A_dstate_stride] * kLog2e;
    const float bias = f.delta_bias ? static_cast<const float*>(f.delta_bias)[dc] : 0.0f;
    const bool softplus = ls_own((int)f.delta_softplus) != 0, bc_vec = ls_own(sg.bc_vec) != 0;
    const int chu = min(dwave, d_end - 1);

    float gg = 0.0f, ag = 0.0f, dsum = 0.0f;                  // g_t of the last token done, a_t g_t, sum of delta
    // raw inputs of a tile (lanes that are off hold an arbitrary valid element: the consumer applies `ok`)
    float n_raw, n_dy, n_z = 0.0f;
    auto fetch = [&](int tile) __attribute__((always_inline)) {
        const int t = tile * kLsT + tk;
        const bool ok = cv && t < L && tile >= tile_lo;
        n_raw = tdl.ld_raw(chu, t, ok);
        n_dy = tdo.ld_raw(chu, t, ok);
        if (HAS_Z) n_z = tz.ld_raw(chu, t, ok);
    };
    fetch(tile_hi - 1);
#pragma unroll 1
    for (int tile = tile_hi - 1; tile >= tile_lo; --tile) {
        const int t0 = tile * kLsT;
        const int t = t0 + tk;
        const bool ok = cv && t < L;
        float Cv[16];
        rC.load16(ls_fresh_kargs(), t0, L, bc_vec && t0 + kLsT <= L, Cv);
        float raw = ok ? n_raw + bias : 0.0f, dy = ok ? n_dy : 0.0f, zf = ok ? n_z : 0.0f;
        asm volatile("" : "+v"(raw), "+v"(dy), "+v"(zf));     // used here: before the next tile's loads are issued
        fetch(tile - 1);
        if (HAS_Z) dy *= zf * sigmoidf_fast(zf);
        float dl = ok ? (softplus ? softplus_ref(raw) : raw) : 0.0f;
        dsum += (t == t_first) ? 0.0f : dl;                   // sum of delta over the segment minus its first token's
        ls_settle(dl, dy);
        ls_arrive(Cv);
        // the sixteen decays first, then the recurrence: left to itself hipcc computes each v_exp_f32 two instructions before
        // its use and every wave sits out the transcendental latency sixteen times per tile (10 cycles per VALU instruction
        // on the SQ counters against 5.4 for the forward's first pass, which has the same operations)
        float a[16];
        sfor<0, 16>([&](auto kc) {
            constexpr int k = decltype(kc)::value;
            a[k] = fast_exp2(tok<k>(dl) * A2);
        });
        ls_arrive(a);
        sfor_down<16>([&](auto kc) {
            constexpr int k = decltype(kc)::value;
            gg = tok_fma<k>(ag, dy, Cv[k]);
            ag = gg * a[k];
        });
    }
    if (!cv) return;                                          // uniform per row; the DPP sums below stay inside a row
    sg.agg[(((int64_t)b * f.dim + d) * sg.S + seg) * NS + n] = gg;
    float dl_nx = 0.0f;
    if (t_next < L) {
        const float raw = tdl.ld(chu, t_next, true) + bias;
        dl_nx = softplus ? softplus_ref(raw) : raw;
    }
    const float tot = ls_row_total(dsum) + dl_nx;
    if (li == 0 && rs == 0) sg.dsum[((int64_t)b * f.dim + d) * sg.S + seg] = tot;
}

// gin[s-1] = exp2(A2 * dsum[s]) * gin[s] + agg[s], right to left (reverse == true), or
// gin[s+1] = exp2(A2 * dsum[s]) * gin[s] + agg[s], left to right (forward): one thread per (batch, channel, state).
// The chain's operands do not depend on the chain: they are fetched 16 segments at a time, all loads in flight
// together (a dependent walk over global memory costs one memory latency per segment).
template <bool REVERSE>
__global__ void __launch_bounds__(256) ssm_ls_carry_kernel(const float* __restrict__ A, int64_t A_d_stride, int64_t A_n_stride,
                                                           int batch, int dim, int N, const LsSeg sg) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)batch * dim * N) return;
    const int n = (int)(i % N);
    const int64_t bd = i / N;
    const int dch = (int)(bd % dim);
    const float A2 = A[dch * A_d_stride + n * A_n_stride] * kLog2e;
    const int S = sg.S;
    float gcur = 0.0f;
    sg.gin[(bd * S + (REVERSE ? S - 1 : 0)) * N + n] = 0.0f;
    // REVERSE: s runs S-1 .. 1 and writes s-1;  forward: s runs 0 .. S-2 and writes s+1
    for (int i0 = 0; i0 < S - 1; i0 += 16) {
        float ag[16], ds[16];
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int idx = i0 + q;
            const int s = REVERSE ? S - 1 - idx : idx;
            const bool ok = idx < S - 1;
            ag[q] = ok ? sg.agg[(bd * S + s) * N + n] : 0.0f;
            ds[q] = ok ? sg.dsum[bd * S + s] : 0.0f;
        }
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int idx = i0 + q;
            if (idx < S - 1) {
                const int s = REVERSE ? S - 1 - idx : idx;
                gcur = fmaf(fast_exp2(A2 * ds[q]), gcur, ag[q]);
                sg.gin[(bd * S + (REVERSE ? s - 1 : s + 1)) * N + n] = gcur;
            }
        }
    }
}

// =========================================================================================================================
// Forward: PASS 1 (end state of a segment for zero inflow, sum of delta) and PASS 2 (outputs and checkpoints).
// One loop over (tile, channel) steps like the backward: the running state of the row's kLsCPR channels lives in
// wave-private LDS (one float per lane and channel), a step's inputs are requested one step ahead, its outputs are stored at
// the start of the next step.  No barrier: waves are independent.
// LEAN (vivim_selective_scan_fwd_lean: a forward no backward follows) is a compile-time twin of PASS 2 without the
// checkpoint store, and without the `out` store when z is given.  `p.x` is then null or a (batch, dim, dstate) fp32
// buffer: the waves of the last segment copy the running state out of LDS after the tile loop -- the state after
// token L - 1, which the full kernel puts into the last checkpoint row.
// =========================================================================================================================
template <typename T, int NS, int PASS, bool HAS_Z, bool LEAN = false>
__global__ void __launch_bounds__(256) ssm_ls_fwd_kernel(const vivim_ssm_fwd_params p, const LsSeg sg) {
    typedef LsGeom<NS> G;
    constexpr int RPS = G::RPS, CPW = G::CPW, CPR = kLsCPR;
    __shared__ float lds_state[4 * CPR * 2 * kWave];          // [wave][channel][h | dsum][lane]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), W = blockDim.x >> 6;
    const int row = lane >> 4, li = lane & 15;
    const int rs = row % RPS, sw = row / RPS;
    const int n = rs * 16 + li;
    const int tk = ((li & 1) << 3) | ((li & 2) << 1) | ((li & 4) >> 1) | ((li & 8) >> 3);
    const int b = blockIdx.y, seg = blockIdx.z;
    const int L = ls_own(p.seqlen), cpg = p.dim / p.n_groups;
    const int cpb = W * CPW;
    const int bpg = (cpg + cpb - 1) / cpb;
    const int g = blockIdx.x / bpg;
    const int d_end = ls_own((g + 1) * cpg);
    const int dwave = ls_own(g * cpg + (blockIdx.x - g * bpg) * cpb + wave * CPW);
    const int rowch = sw * CPR;
    if (dwave >= d_end) return;
    const int ntiles = (L + kLsT - 1) / kLsT;
    const int nck = (ntiles + RPS - 1) / RPS;
    const int blk_lo = seg * sg.seg_blocks, blk_hi = min(nck, blk_lo + sg.seg_blocks);
    const int tile_lo = blk_lo * RPS, tile_hi = min(ntiles, blk_hi * RPS);
    if (PASS == 1 && seg == sg.S - 1) return;                 // the last segment feeds nobody
    typedef vivim_ssm_fwd_params FP;
    LsTensorR<T> tu, tdl;                                     // loaded first in every step: resident
    LsTensor<T> tz, to, toz;
    tu.init(p.u, b * p.u_batch_stride, p.u_d_stride, rowch);
    tdl.init(p.delta, b * p.delta_batch_stride, p.delta_d_stride, rowch);
    if (PASS == 2) {
        to.init(LS_OFF(FP, out), LS_OFF(FP, out_batch_stride), b, p.out_d_stride, rowch);
        if (HAS_Z) {
            tz.init(LS_OFF(FP, z), LS_OFF(FP, z_batch_stride), b, p.z_d_stride, rowch);
            toz.init(LS_OFF(FP, out_z), LS_OFF(FP, out_z_batch_stride), b, p.out_z_d_stride, rowch);
        }
    }
    LsCkpt tx;
    tx.init(LS_OFF(FP, x), b, p.dim, nck, NS, rowch);
    LsRow<T> rB, rC;
    rB.init(LS_OFF(FP, B), LS_OFF(FP, B_batch_stride), b, g, p.B_dstate_stride, n);
    rC.init(LS_OFF(FP, C), LS_OFF(FP, C_batch_stride), b, g, p.C_dstate_stride, n);
    const bool softplus = ls_own((int)p.delta_softplus) != 0, bc_vec = ls_own(sg.bc_vec) != 0;
    float* cstate = lds_state + wave * (CPR * 2 * kWave) + lane;
    static_assert(CPR == 4, "the per-channel registers are selected by hand");

    float A2r[CPR], Dr[CPR], biasr[CPR];
#pragma unroll
    for (int c = 0; c < CPR; ++c) {
        const int d = dwave + rowch + c;
        const bool cv = d < d_end;
        const int dc = cv ? d : d_end - 1;
        A2r[c] = static_cast<const float*>(p.A)[dc * p.A_d_stride + n * p.A_dstate_stride] * kLog2e;
        Dr[c] = p.D ? static_cast<const float*>(p.D)[dc] : 0.0f;
        biasr[c] = p.delta_bias ? static_cast<const float*>(p.delta_bias)[dc] : 0.0f;
        cstate[(c * 2 + 0) * kWave] = (PASS == 2 && sg.S > 1 && cv) ? sg.gin[(((int64_t)b * p.dim + dc) * sg.S + seg) * NS + n] : 0.0f;
        cstate[(c * 2 + 1) * kWave] = 0.0f;
    }
    float n_u, n_raw, n_z = 0.0f;
    auto fetch = [&](int tile, int c) __attribute__((always_inline)) {
        const int t = tile * kLsT + tk;
        const bool ok = dwave + rowch + c < d_end && t < L && tile < tile_hi;
        const int chu = min(dwave + c, d_end - 1);
        n_u = tu.ld_raw(chu, t, ok);
        n_raw = tdl.ld_raw(chu, t, ok);
        if (PASS == 2 && HAS_Z) n_z = tz.ld_raw(ls_fresh_kargs(), chu, t, ok);
    };
    // outputs of the previous step, stored at the start of the next one (see the backward kernel)
    float p_o = 0.0f, p_oz = 0.0f, p_h = 0.0f;
    int p_chu = min(dwave, d_end - 1), p_t = 0, p_ck = 0;
    bool p_st = false, p_ckst = false;
    auto flush = [&]() __attribute__((always_inline)) {
        if (PASS == 2) {
            const ls_kargs qs = ls_fresh_kargs();
            if (!(LEAN && HAS_Z)) to.st(qs, p_chu, p_t, p_st, p_o);
            if (HAS_Z) toz.st(qs, p_chu, p_t, p_st, p_oz);
            if (!LEAN) tx.st(qs, p_chu, p_ck * NS + n, p_ckst, p_h);
        }
    };
    float Bv[16], Cv[16];
    fetch(tile_lo, 0);
#pragma unroll 1
    for (int tile = tile_lo; tile < tile_hi; ++tile) {
        const int t0 = tile * kLsT;
        const int t = t0 + tk;
        const bool tv = t < L;
        {
            const bool vec = bc_vec && t0 + kLsT <= L;
            const ls_kargs q = ls_fresh_kargs();
            rB.load16(q, t0, L, vec, Bv);
            if (PASS == 2) rC.load16(q, t0, L, vec, Cv);
        }
        ls_arrive(Bv);
        if (PASS == 2) ls_arrive(Cv);
        const bool ck_row = PASS == 2 && (((tile + 1) % RPS) == 0 || tile == ntiles - 1);   // a checkpoint row ends here
#pragma unroll 1
        for (int c = 0; c < CPR; ++c) {
            const int d = dwave + rowch + c;
            const bool cv = d < d_end;
            const int chu = min(dwave + c, d_end - 1);
            const bool ok = cv && tv;
            float uu = ok ? n_u : 0.0f, raw = ok ? n_raw : 0.0f, zf = ok ? n_z : 0.0f;
            asm volatile("" : "+v"(uu), "+v"(raw), "+v"(zf)); // used here: before the next step's loads are issued
            flush();
            fetch(c + 1 < CPR ? tile : tile + 1, c + 1 < CPR ? c + 1 : 0);
            const float A2 = c == 0 ? A2r[0] : c == 1 ? A2r[1] : c == 2 ? A2r[2] : A2r[3];
            raw += c == 0 ? biasr[0] : c == 1 ? biasr[1] : c == 2 ? biasr[2] : biasr[3];
            float dl = ok ? (softplus ? softplus_ref(raw) : raw) : 0.0f;                   // fwd_kernel.cuh:153-156
            float w = dl * uu;
            float* cs = cstate + c * 2 * kWave;
            if (PASS == 1) cs[kWave] += dl;
            ls_settle(dl, w);
            float hh = cs[0];
            if (PASS == 1) {
                float a[16];
                sfor<0, 16>([&](auto kc) {
                    constexpr int k = decltype(kc)::value;
                    a[k] = fast_exp2(tok<k>(dl) * A2);                                     // fwd_kernel.cuh:216
                });
                ls_arrive(a);
                sfor<0, 16>([&](auto kc) {
                    constexpr int k = decltype(kc)::value;
                    hh = tok_fma<k>(a[k] * hh, w, Bv[k]);
                });
                cs[0] = hh;
            } else {
                float s[16], z[8], ww[4], v[2], y, a[16];
                sfor<0, 16>([&](auto kc) {
                    constexpr int k = decltype(kc)::value;
                    a[k] = fast_exp2(tok<k>(dl) * A2);
                });
                ls_arrive(a);
                sfor<0, 16>([&](auto kc) {
                    constexpr int k = decltype(kc)::value;
                    hh = tok_fma<k>(a[k] * hh, w, Bv[k]);
                    s[k] = hh * Cv[k];                                                     // fwd_kernel.cuh:256-265
                    ls_reduce_up<k>(s, z, ww, v, y, li);
                });
                cs[0] = hh;
                y = ls_rows_sum<RPS>(y);
                const float Dv = c == 0 ? Dr[0] : c == 1 ? Dr[1] : c == 2 ? Dr[2] : Dr[3];
                const float o = fmaf(Dv, uu, y);
                p_o = o;
                if (HAS_Z) p_oz = o * zf * sigmoidf_fast(zf);                              // fwd_kernel.cuh:280-298
                p_h = hh; p_chu = chu; p_t = t; p_st = ok && rs == 0; p_ck = tile / RPS; p_ckst = ck_row && cv;
            }
        }
    }
    flush();
    if (PASS == 2 && LEAN && tile_hi == ntiles) {             // the last segment: the state after token L - 1
        // (the lane's place is worked out again from the thread index: kept across the tile loop, the row's channel and the
        // state cost the loop five VGPRs and the 16- and 32-state instantiations one wave per SIMD)
        const ls_kargs q = ls_fresh_kargs();
        float* __restrict__ xl = static_cast<float*>(ls_karg<void*>(q, LS_OFF(FP, x)));
        if (xl) {
            int t2 = threadIdx.x;
            asm volatile("" : "+v"(t2));
            const int row2 = (t2 & 63) >> 4;
            const int n2 = (row2 % RPS) * 16 + (t2 & 15), d2 = dwave + (row2 / RPS) * CPR;
            const float* cs2 = lds_state + (t2 >> 6) * (CPR * 2 * kWave) + (t2 & 63);
            xl += ((int64_t)b * ls_karg<int>(q, LS_OFF(FP, dim)) + d2) * NS + n2;
            for (int c = 0; c < CPR; ++c)
                if (d2 + c < d_end) xl[c * NS] = cs2[(c * 2 + 0) * kWave];
        }
    }
    if (PASS == 1) {
        for (int c = 0; c < CPR; ++c) {
            const int d = dwave + rowch + c;
            const float tot = ls_row_total(cstate[(c * 2 + 1) * kWave]);
            if (d >= d_end) continue;
            sg.agg[(((int64_t)b * p.dim + d) * sg.S + seg) * NS + n] = cstate[(c * 2 + 0) * kWave];
            if (li == 0 && rs == 0) sg.dsum[((int64_t)b * p.dim + d) * sg.S + seg] = tot;
        }
    }
}

// =========================================================================================================================
// Host side
// =========================================================================================================================
static size_t ls_bwd_smem(int W, int NS) {
    // per wave: 8 KB of dB / dC slots + the channels' state (4 floats per lane and channel; dstate 32 / 64: + the rebuilt
    // states at the inner tile boundaries of a checkpoint block) + the D / bias table: 50.1 KB for 4 waves at dstate 16
    const int RPS = NS / 16, SPW = 4 / RPS;
    return ((size_t)W * SPW * 2 * NS * 16 + (size_t)W * kLsCPR * (4 + RPS - 1) * kWave + (size_t)W * kLsCPR * 8) * sizeof(float) +
           (size_t)2 * NS * 16 * 4;   // + the staged B / C rows of one tile (sized for fp32)
}

// Calls fn(T{}, LsGeom<NS>{}) for the element type and state count of `f`.
template <typename F> static void with_itype_ns(const vivim_ssm_fwd_params& f, F&& fn) {
    with_itype(f.itype, [&](auto t) {
        switch (f.dstate) {
            case 16: fn(t, LsGeom<16>{}); break;
            case 32: fn(t, LsGeom<32>{}); break;
            case 64: fn(t, LsGeom<64>{}); break;
        }
    });
}

int ls_bwd_occupancy(const vivim_ssm_fwd_params& f, int W) {
    int nb = 3;
    with_itype_ns(f, [&](auto t, auto g) {
        typedef decltype(t) T;
        constexpr int NS = decltype(g)::RPS * 16;
        const size_t smem = ls_bwd_smem(W, NS);
        nb = f.z ? occupancy_query(ssm_ls_bwd_kernel<T, NS, true>, W, smem, 3) : occupancy_query(ssm_ls_bwd_kernel<T, NS, false>, W, smem, 3);
    });
    return nb;
}

static LsSeg ls_seg(void* ws, const vivim_ssm_fwd_params& f, int S, int seg_blocks, bool bc_vec) {
    LsSeg sg = {S, seg_blocks, nullptr, nullptr, nullptr, bc_vec ? 1 : 0};
    if (S > 1) {
        const size_t nbd = (size_t)f.batch * f.dim * S;
        sg.agg = static_cast<float*>(ws);
        sg.gin = sg.agg + nbd * f.dstate;
        sg.dsum = sg.gin + nbd * f.dstate;
    }
    return sg;
}

// Segmented: the pre-pass (recurrence form, or the lanes = tokens closed form the plan picked) + carry; then the main kernel
// of the plan's generation.
void launch_ls_bwd(const vivim_ssm_bwd_params& p, const BwdPlan& q, hipStream_t stream, bool det) {
    const vivim_ssm_fwd_params& f = p.f;
    const LsSeg sg = ls_seg(p.workspace, f, q.S, q.seg, q.bc_vec);
    const int cpg = f.dim / f.n_groups;
    if (q.closed_prepass) launch_bwd_closed_prepass(p, sg, q.K, stream);
    with_itype_ns(f, [&](auto t, auto g) {
        typedef decltype(t) T;
        typedef decltype(g) G;
        constexpr int NS = G::RPS * 16;
        if (sg.S > 1 && !q.closed_prepass) {
            const int PW = 4;                                     // independent waves per pre-pass workgroup, one channel per row
            const int pbpg = (cpg + PW * G::SPW - 1) / (PW * G::SPW);
            const dim3 gpre(pbpg * f.n_groups, f.batch, sg.S - 1);
            if (f.z) hipLaunchKernelGGL((ssm_ls_bwd_prepass_kernel<T, NS, true>), gpre, dim3(PW * kWave), 0, stream, p, sg);
            else     hipLaunchKernelGGL((ssm_ls_bwd_prepass_kernel<T, NS, false>), gpre, dim3(PW * kWave), 0, stream, p, sg);
            const int64_t nthr = (int64_t)f.batch * f.dim * f.dstate;
            hipLaunchKernelGGL((ssm_ls_carry_kernel<true>), dim3((unsigned)((nthr + 255) / 256)), dim3(256), 0, stream,
                               static_cast<const float*>(f.A), f.A_d_stride, f.A_dstate_stride, f.batch, f.dim, f.dstate, sg);
        }
        if (q.ls2) return;
        const int bpg = (cpg + q.W * G::CPW - 1) / (q.W * G::CPW);
        const dim3 grid(bpg * f.n_groups, f.batch, sg.S);
        const size_t smem = ls_bwd_smem(q.W, NS);
        auto launch = [&](auto kernel) {
            allow_smem(kernel, smem);
            hipLaunchKernelGGL(kernel, grid, dim3(q.W * kWave), smem, stream, p, sg);
        };
        if (det) { if (f.z) launch(ssm_ls_bwd_kernel<T, NS, true, true>); else launch(ssm_ls_bwd_kernel<T, NS, false, true>); }
        else     { if (f.z) launch(ssm_ls_bwd_kernel<T, NS, true>);       else launch(ssm_ls_bwd_kernel<T, NS, false>); }
    });
    if (q.ls2) launch_ls2_bwd(p, sg, q.W, stream, det);
}

void launch_ls_fwd(const vivim_ssm_fwd_params& p, const FwdPlan& q, hipStream_t stream, bool lean) {
    const LsSeg sg = ls_seg(p.workspace, p, q.S, q.seg, q.bc_vec);
    const int cpg = p.dim / p.n_groups;
    const int PW = 4;
    with_itype_ns(p, [&](auto t, auto g) {
        typedef decltype(t) T;
        typedef decltype(g) G;
        constexpr int NS = G::RPS * 16;
        const int bpg = (cpg + PW * G::CPW - 1) / (PW * G::CPW);
        const dim3 grid(bpg * p.n_groups, p.batch, sg.S), block(PW * kWave);
        if (sg.S > 1) {
            hipLaunchKernelGGL((ssm_ls_fwd_kernel<T, NS, 1, false>), grid, block, 0, stream, p, sg);
            const int64_t nthr = (int64_t)p.batch * p.dim * p.dstate;
            hipLaunchKernelGGL((ssm_ls_carry_kernel<false>), dim3((unsigned)((nthr + 255) / 256)), dim3(256), 0, stream,
                               static_cast<const float*>(p.A), p.A_d_stride, p.A_dstate_stride, p.batch, p.dim, p.dstate, sg);
        }
        if (lean) {
            if (p.z) hipLaunchKernelGGL((ssm_ls_fwd_kernel<T, NS, 2, true, true>), grid, block, 0, stream, p, sg);
            else     hipLaunchKernelGGL((ssm_ls_fwd_kernel<T, NS, 2, false, true>), grid, block, 0, stream, p, sg);
        } else {
            if (p.z) hipLaunchKernelGGL((ssm_ls_fwd_kernel<T, NS, 2, true>), grid, block, 0, stream, p, sg);
            else     hipLaunchKernelGGL((ssm_ls_fwd_kernel<T, NS, 2, false>), grid, block, 0, stream, p, sg);
        }
    });
}

}  // namespace vivim
