// scan_plan.hip -- which selective-scan kernels run, on what cut of the token axis, with how much workspace (scan_plan.cuh).
#include <stdlib.h>
#include <algorithm>
#include <atomic>
#include "scan_plan.cuh"
#include "capi.cuh"

namespace vivim {

const ScanEnv& scan_env() {
    static const ScanEnv e = [] {
        auto num = [](const char* name, int dflt) { const char* v = getenv(name); return v ? atoi(v) : dflt; };
        // VIVIM_CHAN_WAVES default 2048: swept 512 ... 8192 on the grouped cfg-2 shapes (309/144/106/64 us at 2048;
        // 377/198/130/68 at 1024; 320/167/125/70 at 4096); again with the packed token update: 293/146/101/69 at 1536,
        // 283/141/104/70 at 2048, 300/164/115/70 at 3072, 304/165/124/70 at 4096
        return ScanEnv{num("VIVIM_CHAN_WAVES", 2048), num("VIVIM_CHAN_XCD", -1)};
    }();
    return e;
}

static int cu_count() {
    static const int n = [] {
        int dev = 0, v = 0;
        if (hipGetDevice(&dev) != hipSuccess ||
            hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || v <= 0)
            v = 256;                                    // MI355X; also what a GPU-less build host reports
        return v;
    }();
    return n;
}

// Resident workgroups per CU of the lanes = states backward instantiation that `f` selects (registers and LDS differ between
// instantiations: 2 or 3 waves per SIMD), cached by (generation, itype, dstate, z, W).  Filled from whichever thread
// plans first (the autograd worker included): relaxed atomics, a racing fill stores the same value.
static int ls_bwd_blocks_per_cu(const vivim_ssm_fwd_params& f, int W, bool ls2) {
    static std::atomic<int> cache[2][3][3][2][5];
    if (f.itype < 0 || f.itype > 2) return ls2 ? 2 : 3;      // (a workspace query with a bad itype: what a build host answers)
    std::atomic<int>& c = cache[ls2][f.itype][f.dstate / 32][f.z != nullptr][W];
    int nb = c.load(std::memory_order_relaxed);
    if (nb == 0) {
        nb = ls2 ? ls2_bwd_occupancy(f, W) : ls_bwd_occupancy(f, W);
        c.store(nb, std::memory_order_relaxed);
    }
    return nb;
}

// ---- vector rows -------------------------------------------------------------------------------------------------------
// Rows read or written with unconditional epv-element vectors: the base 16-byte (epv * es-byte) aligned and every stride a
// whole number of vectors.  `ptr` null (or a shape-only query) checks the strides alone.
static bool rows_vec_ok(const void* ptr, std::initializer_list<int64_t> strides, int64_t epv, int es) {
    if (reinterpret_cast<uintptr_t>(ptr) % (uintptr_t)(epv * es)) return false;
    for (int64_t s : strides)
        if (s % epv) return false;
    return true;
}
// the forward's activation rows: u, delta, out (+ z, out_z)
static bool fwd_rows_vec_ok(const vivim_ssm_fwd_params& f, int64_t epv, bool ptrs = true) {
    const int es = elem_bytes(f.itype);
    auto P = [&](const void* q) { return ptrs ? q : nullptr; };
    return rows_vec_ok(P(f.u), {f.u_batch_stride, f.u_d_stride}, epv, es) &&
           rows_vec_ok(P(f.delta), {f.delta_batch_stride, f.delta_d_stride}, epv, es) &&
           rows_vec_ok(P(f.out), {f.out_batch_stride, f.out_d_stride}, epv, es) &&
           (!f.z || (rows_vec_ok(P(f.z), {f.z_batch_stride, f.z_d_stride}, epv, es) &&
                     rows_vec_ok(P(f.out_z), {f.out_z_batch_stride, f.out_z_d_stride}, epv, es)));
}
static bool b_rows_vec_ok(const vivim_ssm_fwd_params& f, int64_t epv) {
    return rows_vec_ok(f.B, {f.B_batch_stride, f.B_group_stride, f.B_dstate_stride}, epv, elem_bytes(f.itype));
}
static bool c_rows_vec_ok(const vivim_ssm_fwd_params& f, int64_t epv) {
    return rows_vec_ok(f.C, {f.C_batch_stride, f.C_group_stride, f.C_dstate_stride}, epv, elem_bytes(f.itype));
}
// the backward's activation rows: u, delta, dout, du, ddelta (+ z, out, dz, out_z when given)
static bool bwd_rows_vec_ok(const vivim_ssm_bwd_params& p, int64_t epv) {
    const vivim_ssm_fwd_params& f = p.f;
    const int es = elem_bytes(f.itype);
    return rows_vec_ok(f.u, {f.u_batch_stride, f.u_d_stride}, epv, es) &&
           rows_vec_ok(f.delta, {f.delta_batch_stride, f.delta_d_stride}, epv, es) &&
           rows_vec_ok(p.dout, {p.dout_batch_stride, p.dout_d_stride}, epv, es) &&
           rows_vec_ok(p.du, {p.du_batch_stride, p.du_d_stride}, epv, es) &&
           rows_vec_ok(p.ddelta, {p.ddelta_batch_stride, p.ddelta_d_stride}, epv, es) &&
           (!f.z || (rows_vec_ok(f.z, {f.z_batch_stride, f.z_d_stride}, epv, es) &&
                     rows_vec_ok(f.out, {f.out_batch_stride, f.out_d_stride}, epv, es) &&
                     rows_vec_ok(p.dz, {p.dz_batch_stride, p.dz_d_stride}, epv, es) &&
                     (!f.out_z || rows_vec_ok(f.out_z, {f.out_z_batch_stride, f.out_z_d_stride}, epv, es))));
}

// ---- lanes = states shapes ---------------------------------------------------------------------------------------------
// Variable B / C, a state count that fills whole 16-lane rows, and (channel, token) byte offsets inside one batch element
// that fit the 32-bit offsets of the buffer accesses (sizes and strides only).
static bool ls_span_ok(int64_t rows, int64_t row_stride, int64_t len, int es) {
    return row_stride >= 0 && ((rows - 1) * row_stride + len) * es < (int64_t)0xffff0000;
}
static bool ls_shape_ok(const vivim_ssm_fwd_params& f) {
    if (!(f.is_variable_B && f.is_variable_C && (f.dstate == 16 || f.dstate == 32 || f.dstate == 64) && f.dim % f.n_groups == 0))
        return false;
    const int es = elem_bytes(f.itype);
    // (the resource's size field carries the channel, 0xffff0000 + chu, and a lane that is off stores at offset 0xfffffff0,
    // which must stay >= that size: chu < 65520)
    if (f.dim > 65520 || !ls_span_ok(f.dim, f.u_d_stride, f.seqlen, es) || !ls_span_ok(f.dim, f.delta_d_stride, f.seqlen, es) ||
        !ls_span_ok(f.dstate, f.B_dstate_stride, f.seqlen, es) || !ls_span_ok(f.dstate, f.C_dstate_stride, f.seqlen, es) ||
        !ls_span_ok(f.dim, (int64_t)((f.seqlen + 15) / 16) * f.dstate, 0, 4))
        return false;
    if (f.z && (!ls_span_ok(f.dim, f.z_d_stride, f.seqlen, es))) return false;
    return true;
}
static int ls_ckpt_len(const vivim_ssm_fwd_params& f) { return 16 * (f.dstate / 16); }

// Which checkpoint rows a shape gets -- and with them which backward family (the forward families that can write them
// follow).  Measured on MI355X (tools/kb_round2.sh, profiles/r02_kbench_families.log), lanes = states against the round-1
// families at dstate 16: the backward wins on short rows (cfg 2 grouped stages 1-3: 273 / 172 / 84 us against 288 / 185 /
// 149) and loses a few per cent on long ones (L 20480: 592 against 564 us; L 81920: 2214 against 2111), where the
// lanes = tokens kernel amortises its scans over 512-token steps; at dstate 32 / 64 its extra forward sweep per checkpoint
// block costs more than it gains (cfg 5: 1018 against 820 us).  Forward tuning 5 / 6 pin the short rows for any such shape.
static bool ls_rows(const vivim_ssm_fwd_params& f) {
    if (!ls_shape_ok(f)) return false;
    const int t = tuning_fwd_variant();
    if (t == kFwdChan || t == kFwdStates) return true;
    if (t != kFwdAuto) return false;
    // Round 3: with the second-generation lanes = states backward (scan_ls2.hip) and the closed-form pre-pass the two backward
    // families take the same time on long 16-bit rows (cfg 2 grouped stage 0: 547-561 against 555-588 us) while the lanes =
    // states one moves half the bytes (0.58 against 1.08 GB per launch); the forward pays 20 us there for the denser
    // checkpoints (262 against 242).  fp32 rows keep the old limit: the denser checkpoints cost the forward 15 % (cfg 3
    // grouped stage 0: 2974 against 2586 us) for 4 % of the backward.
    return f.dstate == 16 && f.seqlen <= (f.itype == VIVIM_F32 ? 8192 : 32768);
}

// Tokens per checkpoint row of x.  The lanes = states backward (scan_ls.hip) rebuilds the forward states of a 16-token tile
// from a checkpoint, so every shape it takes gets one row per 16 * (dstate / 16) tokens, written by the lanes = channels
// and lanes = states forward kernels; the n-split / generic kernels write one row per kChunk tokens (two per 512-token
// n-split step) and are only reached for other shapes or when the tuning selector pins them.  A pure function of the
// shape and of the forward tuning value: forward and backward calls must see the same one.
static int scan_ckpt_len(const vivim_ssm_fwd_params& f) { return ls_rows(f) ? ls_ckpt_len(f) : kChunk; }
static int scan_chunk_len(int) { return kChunk; }

// Token-axis cut of the lanes = states kernels.  All workgroups of a launch take about the same time, so the launch runs in
// rounds of the resident workgroups; one workgroup over a whole number of rounds costs a full extra round (the first build
// cut cfg 2 into 774 workgroups for 768 slots and took twice the time).  So: as many segments as FIT in `slots` waves (a
// whole number of rounds when even one segment does not fit), whole checkpoint blocks per segment, at least `min_blocks` of
// them so that a segment's prologue and the pre-pass stay a small part of it.
static void ls_segmentation(const vivim_ssm_fwd_params& f, int waves_per_seg, int slots, int min_blocks, int& S, int& seg_blocks) {
    const int nck = (f.seqlen + ls_ckpt_len(f) - 1) / ls_ckpt_len(f);
    int s = slots / waves_per_seg;                             // one round
    const int smax = nck / min_blocks;
    if (s > smax) s = smax;
    if (s > 512) s = 512;
    if (s < 1) s = 1;
    seg_blocks = (nck + s - 1) / s;
    S = (nck + seg_blocks - 1) / seg_blocks;
}
// segment scratch of the lanes = states and lanes = tokens families: agg, gin per (batch, channel, segment, state), dsum
static size_t seg_ws_bytes(const vivim_ssm_fwd_params& f, int S) {
    return S > 1 ? (size_t)f.batch * f.dim * S * (2 * f.dstate + 1) * sizeof(float) : 0;
}
static bool ws_ok(const void* ws, int64_t bytes, size_t need) { return need && ws && (size_t)bytes >= need; }

// ---- forward -----------------------------------------------------------------------------------------------------------
// Lanes = channels, sizes and tuning only.  Automatic choice, from tools/kbench.py on MI355X (us, this family vs n-split;
// cols = batch * dim / 64 waves' worth of channels, work = cols * seqlen wave-tokens):
//   grouped v3 stages 0-3 (cols 18/36/90/144, work 368k/184k/115k/46k): 309/140/104/64 vs 369/159/112/68
//   per-direction stages 0-3 (cols 6/12/30/48, work 123k/61k/38k/15k):  135/84/60/37  vs 131/65/39/29
//   cfg 3 stage 0 fp32 (cols 16, work 1.3M): 997 vs 1189;  grouped (cols 48, 3.9M): 2883 vs 3453
// -> enough total work AND enough independent channel blocks; otherwise the two passes + carry are latency-bound
// and n-split wins.  Tuning 5 forces this family, any other non-zero value excludes it.
static bool chan_shape_ok(const vivim_ssm_fwd_params& f, int ck) {
    if (!f.is_variable_B || !f.is_variable_C || (f.dstate != 16 && f.dstate != 64) || f.seqlen % 8 != 0) return false;
    if (f.dim % f.n_groups != 0 || (f.dim / f.n_groups) % kWave != 0) return false;   // whole 64-channel blocks per group
    const int tune = tuning_fwd_variant();
    if (tune != kFwdChan) {
        if (tune != kFwdAuto) return false;
        if (f.dstate == 64 && f.itype == VIVIM_F32) return false;   // 255 + 4 registers: one wave per SIMD (n-split is faster)
        const int64_t cols = (int64_t)f.batch * (f.dim / kWave);
        // short checkpoint rows: the alternative is the lanes = states forward, which wins below ~150 k wave-tokens (cfg 2
        // grouped stages 1-3, 184 k / 115 k / 46 k: 150 / 98 / 51 us against 137 / 100 / 59 with 64-byte tile rows; cfg 3
        // stage 2, 410 k: 361 against 302)
        const int64_t least = ck < kChunk ? 150000 : 110000;
        if (cols < 8 || cols * f.seqlen < least) return false;
    }
    return fwd_rows_vec_ok(f, vec_elems(f.itype), false);
}
// segments of whole tiles for about scan_env().chan_waves waves in flight; the fp32 B / C copy, then the carries
static size_t chan_layout(const vivim_ssm_fwd_params& f, FwdPlan& q) {
    const int tt = f.itype == VIVIM_F32 ? ChTile<float>::TT : ChTile<bf16_t>::TT;
    const int ntiles = (f.seqlen + tt - 1) / tt;
    const int64_t waves = (int64_t)((f.dim / f.n_groups + kWave - 1) / kWave) * f.n_groups * f.batch;
    int64_t want = (scan_env().chan_waves + waves - 1) / waves;
    if (want > ntiles) want = ntiles;
    if (want > 512) want = 512;       // the carry kernel keeps a whole chain in LDS: 512 * 17 * 4 = 34 KB
    if (want < 1) want = 1;
    q.seg = (int)((ntiles + want - 1) / want);
    q.S = (ntiles + q.seg - 1) / q.seg;
    q.Lpad = ntiles * tt;
    q.bc_floats = (size_t)f.batch * f.n_groups * (q.Lpad + 1) * 32 * (f.dstate / 16);
    const size_t h_floats = q.S > 1 ? (size_t)f.batch * f.dim * q.S * (f.dstate + 1) : 0;
    return (q.bc_floats + h_floats) * sizeof(float);
}
// the lanes = states forward / pre-pass kernels: 7 - 8 waves per SIMD (<= 72 VGPRs), no LDS, whole 4-wave workgroups
static void ls_fwd_segmentation(const vivim_ssm_fwd_params& f, int& S, int& seg_blocks) {
    const int cpw = (4 / (f.dstate / 16)) * kLsCPR;
    const int cpg = f.dim / f.n_groups;
    const int waves_per_seg = ((cpg + 4 * cpw - 1) / (4 * cpw)) * 4 * f.n_groups * f.batch;
    ls_segmentation(f, waves_per_seg, cu_count() * 28, 4, S, seg_blocks);
}

// launch = false: the shape level (ck, ws); true: also the family and its segmentation for this call's pointers.
static FwdPlan plan_scan_fwd(const vivim_ssm_fwd_params& f, bool launch) {
    FwdPlan q{};
    const bool states = ls_rows(f);
    q.ck = states ? ls_ckpt_len(f) : kChunk;
    // either of two families may run (the lanes = channels one also wants aligned rows, known only at launch): the larger
    const bool chan = chan_shape_ok(f, q.ck);
    const size_t chan_ws = chan ? chan_layout(f, q) : 0;
    int lsS = 1, ls_seg = 0;
    if (states) ls_fwd_segmentation(f, lsS, ls_seg);
    const size_t ls_ws = states ? seg_ws_bytes(f, lsS) : 0;
    q.ws = chan_ws > ls_ws ? chan_ws : ls_ws;
    if (!launch) return q;

    // lanes = channels: long, wide problems (or tuning 5); either row length
    if (chan && fwd_rows_vec_ok(f, vec_elems(f.itype)) && f.workspace && (size_t)f.workspace_bytes >= chan_ws &&
        (reinterpret_cast<uintptr_t>(f.workspace) & 63) == 0) {
        // Measured, VIVIM_CHAN_XCD=0 / 1 (profiles/r02_chan_xcd_ab.log): the re-numbering gains 2 - 5 % on the bf16 grouped
        // shapes and where two workgroups share a group's B / C rows (cfg 3 stage 1), and loses 2 - 10 % on fp32 problems
        // with one workgroup per group (cfg 3 stage 0: 831 -> 845 us; grouped 2563 -> 2807 us).
        const int wg_per_group = ((f.dim / f.n_groups) / kWave + kChWaves - 1) / kChWaves;
        q.xcd = scan_env().chan_xcd >= 0 ? scan_env().chan_xcd : ((wg_per_group >= 2 || f.itype != VIVIM_F32) ? 1 : 0);
        q.family = FwdFamily::chan;
        return q;
    }
    if (states) {                                           // lanes = states (short checkpoint rows)
        // out / out_z normally inherit delta's / z's strides, which ls_shape_ok has already accepted; otherwise the call
        // is "not implemented"
        const int es = elem_bytes(f.itype);
        if (!ls_span_ok(f.dim, f.out_d_stride, f.seqlen, es) || (f.z && !ls_span_ok(f.dim, f.out_z_d_stride, f.seqlen, es)))
            return q;
        q.family = FwdFamily::states;
        q.bc_vec = b_rows_vec_ok(f, vec_elems(f.itype)) && c_rows_vec_ok(f, vec_elems(f.itype));
        const bool seg = ws_ok(f.workspace, f.workspace_bytes, ls_ws);
        q.S = seg ? lsS : 1;
        q.seg = seg ? ls_seg : (f.seqlen + q.ck - 1) / q.ck;
        return q;
    }
    // n-split: 8 waves per workgroup, dstate / 8 states per wave.  The kernel uses unconditional 16-byte vectors: every row
    // must be 16-byte aligned and the sequence a whole number of 8-token lanes; anything else takes the generic kernel.
    q.family = FwdFamily::generic;
    const int epv = vec_elems(f.itype);
    if (!f.is_variable_B || !f.is_variable_C || f.dstate % 8 != 0 || f.seqlen % 8 != 0 || !fwd_rows_vec_ok(f, epv) ||
        !b_rows_vec_ok(f, epv) || !c_rows_vec_ok(f, epv))
        return q;
    // 512-token steps (K=8) halve the per-step fixed cost; 256-token steps (K=4) need 100 instead of 160 VGPRs, so several
    // workgroups share a CU -- better once there are enough workgroups to fill the chip twice AND the rows are short (few
    // steps per row: finer steps waste less of the last one).  Measured at the grouped v3 shapes (dim = 3 * d_inner,
    // tools/kbench.py --groups 3): K=8 wins for long rows (L 20480: 365 vs 503 us, L 5120: 160 vs 188 us), K=4 for short
    // ones (L 1280: 112 vs 130 us, L 320: 68 vs 87 us).  Tuning 1 / 2 / 3 pin K=8 / K=4 / the generic kernel.
    const int t = tuning_fwd_variant();
    const int64_t nwg = (int64_t)((f.dim / f.n_groups + kNsR - 1) / kNsR) * f.n_groups * f.batch;
    const int v = (t != kFwdAuto && t < kFwdChan) ? t : ((nwg >= 512 && f.seqlen < 4096) ? kFwdNsplitK4 : kFwdNsplitK8);
    if (v == kFwdGeneric) return q;
    q.family = FwdFamily::nsplit;
    q.K = v == kFwdNsplitK4 ? 4 : 8;
    return q;
}

static size_t scan_fwd_workspace_bytes(const vivim_ssm_fwd_params& f) { return plan_scan_fwd(f, false).ws; }

// The launches of plan q on p, full or lean; false: no family is built for it.
static bool launch_fwd_plan(const vivim_ssm_fwd_params& p, const FwdPlan& q, hipStream_t s, bool lean) {
    switch (q.family) {
        case FwdFamily::chan: launch_fwd_chan(p, q, s, lean); return true;
        case FwdFamily::states: launch_ls_fwd(p, q, s, lean); return true;
        case FwdFamily::nsplit: launch_fwd_nsplit(p, q, s, lean); return true;
        case FwdFamily::generic: launch_fwd_generic(p, s, lean); return true;
        case FwdFamily::none: break;
    }
    return false;
}

static bool ssm_fwd_dispatch(const vivim_ssm_fwd_params& p, hipStream_t s) { return launch_fwd_plan(p, plan_scan_fwd(p, true), s, false); }

// The lean forward (vivim_selective_scan_fwd_lean): no checkpoints, no `out` beside `out_z`.  It is planned as the full call
// on the same tensors would be -- same family, same cut of the token axis, hence the same bits -- with the `out` the full
// call would have been given: one laid out like delta (what both Python wrappers allocate).  The kernels get `last_state`
// (null, or fp32 (batch, dim, dstate)) in the place of `x`.
static bool ssm_fwd_lean_dispatch(const vivim_ssm_fwd_params& p, void* last_state, hipStream_t s) {
    vivim_ssm_fwd_params f = p;
    if (p.z) {
        f.out = const_cast<void*>(p.delta);          // (planning only: nothing is written through it)
        f.out_batch_stride = p.delta_batch_stride;
        f.out_d_stride = p.delta_d_stride;
    }
    const FwdPlan q = plan_scan_fwd(f, true);
    f = p;
    f.x = last_state;
    return launch_fwd_plan(f, q, s, true);
}

// ---- backward ----------------------------------------------------------------------------------------------------------
// Lanes = states workgroup width: 16 * W channels (dstate 16) of one group share the dB / dC reduction.
static int ls_bwd_waves(const vivim_ssm_fwd_params& f) {
    const int cpw = (4 / (f.dstate / 16)) * kLsCPR;
    const int w = (f.dim / f.n_groups + cpw - 1) / cpw;
    // (8 waves = one workgroup per 128-channel group, plain dB / dC stores instead of two atomic contributions, measured
    // SLOWER with the second-generation kernel: 583 against 557 us at cfg 2 grouped stage 0, 6466 against 5481 at cfg 3 --
    // one workgroup per CU has nobody to run while it waits at its barriers)
    return w > 4 ? 4 : w;
}

// Lanes = tokens, tokens per lane.  Most of a state iteration is scan machinery whose cost does not depend on K (DESIGN.md
// 4.3), so 8 tokens per lane (512-token steps, 229-243 VGPRs of the 256 available at two waves per SIMD, no scratch) nearly
// halve the instructions per state update: measured -4 ... -25 % on Vivim's bf16 shapes, -4 ... -9 % on the fp32 ones --
// except where the last 512-token step would be mostly empty (L = 1280: three steps, 20 % of the slots idle, +6 % against
// five full 256-token steps).
static int bwd_tokens_per_lane(int seqlen) {
    const int64_t slots8 = (int64_t)((seqlen + 511) / 512) * 512, slots4 = (int64_t)((seqlen + 255) / 256) * 256;
    return slots8 * 100 > slots4 * 115 ? 4 : 8;
}

// Lanes = tokens, how the token axis is cut.  One 8-wave workgroup is resident per CU and all workgroups of a launch take the
// same time, so the launch runs in rounds of `ncu` workgroups: cost(S) ~ ceil(base * S / ncu) * (ceil(nsteps / S) + fixed),
// with base = workgroups before the split and `fixed` ~ 0.3 step for a workgroup's prologue / final reductions.  Measured
// against the former fixed target of 1024 workgroups: per-direction stage 0 287 -> 243 us (S 40 -> 10), grouped stage 2
// 255 -> 227 us (S 3 -> 2); grouped stage 0 unchanged (S 14 -> 7..10).  Ties go to the smaller S (less pre-pass).
// Minimises rounds-of-the-chip x (steps per segment + fixed cost) for workgroups of W waves; returns the workgroups.
static int64_t bwd_segmentation(const vivim_ssm_fwd_params& f, int K, int W, int& S, int& seg_steps) {
    const int tile = kWave * K;
    const int nsteps = (f.seqlen + tile - 1) / tile;
    const int ppg = (f.dim / f.n_groups + kBwR - 1) / kBwR;
    const int64_t base = (int64_t)((ppg + W - 1) / W) * f.n_groups * f.batch;
    // workgroups in flight per CU: two waves per SIMD at K = 8 (240-248 VGPRs), three at K = 4 with 4-wave workgroups (145)
    const int slots = cu_count() * (K == 4 && W == 4 ? 3 : kBwWmax / W);
    int best = 1;
    double best_cost = 1e300;
    for (int s = 1; s <= nsteps && s <= 64; ++s) {
        const int steps = (nsteps + s - 1) / s;
        if ((nsteps + steps - 1) / steps != s) continue;            // not a distinct cut
        const double rounds = (double)((base * s + slots - 1) / slots);
        // a cut adds the pre-pass over all segments but the first (~0.4 of a main-pass step per step) and the carry kernel
        const double cost = rounds * (steps * (1.0 + 0.4 * (s - 1) / s) + 0.3);
        if (cost < best_cost - 1e-9) { best_cost = cost; best = s; }
    }
    seg_steps = (nsteps + best - 1) / best;
    S = (nsteps + seg_steps - 1) / seg_steps;
    return base * S;
}

// `p` null: the shape level (ck, ws); otherwise also the family and its segmentation for this call's pointers.
static BwdPlan plan_scan_bwd(const vivim_ssm_fwd_params& f, const vivim_ssm_bwd_params* p) {
    BwdPlan q{};
    q.ck = scan_ckpt_len(f);
    const int tv = tuning_bwd_variant();
    // The lanes = states family (scan_ls.hip) takes every shape whose checkpoints were written for it, unless the tuning
    // selector pins one of the lanes = tokens kernels (1 / 2: fast kernel with 8 / 4 waves, 3: generic).
    if (ls_shape_ok(f) && q.ck == ls_ckpt_len(f) && (tv == kBwdAuto || tv == kBwdStates1 || tv == kBwdStates2)) {
        // Which main kernel a shape gets is decided from sizes alone: dstate 16 and tuning 0 / 5 take the second generation,
        // 4 the first.  A call whose rows then fail its vector checks runs the first generation on the same segmentation.
        const bool ls2_wanted = f.dstate == 16 && f.seqlen % vec_elems(f.itype) == 0 && (tv == kBwdAuto || tv == kBwdStates2);
        q.W = ls_bwd_waves(f);
        const int cpw = (4 / (f.dstate / 16)) * kLsCPR;
        const int bpg = (f.dim / f.n_groups + q.W * cpw - 1) / (q.W * cpw);
        ls_segmentation(f, bpg * q.W * f.n_groups * f.batch, cu_count() * ls_bwd_blocks_per_cu(f, q.W, ls2_wanted) * q.W, 4,
                        q.S, q.seg);
        // Long segments are cut at multiples of 256 tokens, so that the lanes = tokens pre-pass (closed form, 16-byte vector
        // loads) can stand in for the recurrence form.
        const int nck = (f.seqlen + 15) / 16;
        if (ls2_wanted && q.S > 1 && q.seg >= 12) {
            q.seg = (q.seg + 8) / 16 * 16;
            q.S = (nck + q.seg - 1) / q.seg;
        }
        q.ws = seg_ws_bytes(f, q.S);
        if (!p) return q;
        q.family = BwdFamily::generic;                     // (reads the short checkpoint rows)
        {   // the tensors only the backward sees
            const int es = elem_bytes(f.itype);
            if (f.x == nullptr || !ls_span_ok(f.dim, p->dout_d_stride, f.seqlen, es) ||
                !ls_span_ok(f.dim, p->du_d_stride, f.seqlen, es) || !ls_span_ok(f.dim, p->ddelta_d_stride, f.seqlen, es))
                return q;
            if (f.z && (!ls_span_ok(f.dim, f.out_d_stride, f.seqlen, es) || !ls_span_ok(f.dim, p->dz_d_stride, f.seqlen, es) ||
                        (f.out_z && !ls_span_ok(f.dim, f.out_z_d_stride, f.seqlen, es))))
                return q;
        }
        q.family = BwdFamily::states;
        if (!ws_ok(p->workspace, p->workspace_bytes, q.ws)) {
            q.S = 1;
            q.seg = (f.seqlen + ls_ckpt_len(f) - 1) / ls_ckpt_len(f);
        }
        const int epv = vec_elems(f.itype);
        q.bc_vec = b_rows_vec_ok(f, epv) && c_rows_vec_ok(f, epv);
        q.ls2 = ls2_wanted && bwd_rows_vec_ok(*p, epv);
        // The closed-form pre-pass (ssm_bwd_prepass_kernel) reads delta, dout, z and C with K-token vectors.  Measured: half
        // the time of the recurrence form (cfg 3 grouped stage 0: 989 against 1931 us).
        q.K = (q.seg * 16) % 512 == 0 && f.seqlen % 8 == 0 ? 8 : 4;
        const int es = elem_bytes(f.itype), pv = (q.K * es >= 16 ? 16 : q.K * es) / es;
        q.closed_prepass = q.S > 1 && q.ls2 && (q.seg * 16) % 256 == 0 && f.seqlen % q.K == 0 &&
                           rows_vec_ok(f.delta, {f.delta_batch_stride, f.delta_d_stride}, pv, es) &&
                           rows_vec_ok(p->dout, {p->dout_batch_stride, p->dout_d_stride}, pv, es) &&
                           (!f.z || rows_vec_ok(f.z, {f.z_batch_stride, f.z_d_stride}, pv, es)) && c_rows_vec_ok(f, pv);
        return q;
    }
    if (f.is_variable_B && f.is_variable_C && f.dstate <= 64) {
        // Lanes = tokens, waves per workgroup.  Eight waves share one B/C tile and one set of dB/dC atomics (half as many
        // atomics per address as two 4-wave workgroups) and win on short rows that fit the chip in one round (D 1024, L 320:
        // 55 us with 8 waves, 73 us with 4; D 640, L 1280: 96 vs 102 us).  Two independent 4-wave workgroups per CU win
        // when a workgroup walks several steps -- one runs while the other waits at its per-state barrier -- and past one
        // round, where the last round is cut finer (MI355X, cfg 2 grouped stages 0-3: 597/314/225/147 -> 583/293/198/145
        // us; cfg 3 stages 0-2: 2241/1103/779 -> 2151/981/625 us).  Tuning 1 / 2 pins 8 / 4.
        q.K = bwd_tokens_per_lane(f.seqlen);
        q.W = kBwWmax;
        const int64_t wgs = bwd_segmentation(f, q.K, q.W, q.S, q.seg);
        if (tv == kBwdTokensW4 || (tv != kBwdTokensW8 && (wgs > cu_count() || q.seg >= 4))) {
            q.W = 4;
            bwd_segmentation(f, q.K, q.W, q.S, q.seg);
        }
        q.ws = seg_ws_bytes(f, q.S);
    }
    if (!p) return q;
    q.family = BwdFamily::generic;
    // the fast kernel reads one checkpoint row per kChunk tokens, with unconditional K-element vectors: rows aligned to the
    // vector size, seqlen a whole number of lanes
    const int es = elem_bytes(f.itype), epv = (q.K * es >= 16 ? 16 : q.K * es) / es;
    if (!q.K || f.x == nullptr || tv == kBwdGeneric || q.ck != kChunk || f.seqlen % q.K != 0 || !bwd_rows_vec_ok(*p, epv) ||
        !b_rows_vec_ok(f, epv) || !c_rows_vec_ok(f, epv))
        return q;
    q.family = BwdFamily::tokens;
    if (!ws_ok(p->workspace, p->workspace_bytes, q.ws)) {
        q.S = 1;
        q.seg = (f.seqlen + kWave * q.K - 1) / (kWave * q.K);
    }
    // per-lane dA partials in LDS pay off once a workgroup walks several steps (grouped stage 0, 6 steps: 724 -> 698 us);
    // for one or two steps their zero-fill and final reduction cost more than the per-state wave reductions they replace
    // (stage 3: 74 -> 80 us)
    q.da_lds = f.dstate <= 16 && q.seg >= 2;
    return q;
}

static size_t scan_bwd_workspace_bytes(const vivim_ssm_fwd_params& f) { return plan_scan_bwd(f, nullptr).ws; }

// ---- deterministic backward (vivim_selective_scan_bwd_det; slot scheme in det.cuh) ----
// Slots per family: dA / dD / dbias one per (batch, segment) -- the generic kernel has no segments; dB / dC one per
// workgroup (lanes = tokens) or channel set (generic) of a B/C group, in a (batch, group, dstate, seqlen) slot.  Constant
// dB / dC (generic only) take one (dim, dstate) slot per batch.  The lanes = states kernels keep their dB / dC adds while
// a group has at most two workgroups.
// The lanes = tokens kernel at 8 tokens per lane has no VGPR left for the slot stores with two waves per SIMD: the
// deterministic call runs it with 4-wave workgroups (one per CU), re-segmented for that width.
static void det_tokens_width(const vivim_ssm_fwd_params& f, const vivim_ssm_bwd_params* p, BwdPlan& q) {
    if (q.K != 8 || q.W != kBwWmax) return;
    q.W = 4;
    bwd_segmentation(f, q.K, q.W, q.S, q.seg);
    q.ws = seg_ws_bytes(f, q.S);
    if (p && q.family == BwdFamily::tokens) {
        if (!ws_ok(p->workspace, p->workspace_bytes, q.ws)) {
            q.S = 1;
            q.seg = (f.seqlen + kWave * q.K - 1) / (kWave * q.K);
        }
        q.da_lds = f.dstate <= 16 && q.seg >= 2;
    }
}

struct ScanDetLayout {
    int64_t nA, nB, eB;            // slots of dA / dD / dbias; slots of dB / dC and floats per slot (nB 0: not slotted)
    size_t bytes;
};
static ScanDetLayout scan_det_layout(const vivim_ssm_fwd_params& f, BwdFamily fam, int S, int W) {
    const int64_t cpg = f.dim / f.n_groups, bgnl = (int64_t)f.batch * f.n_groups * f.dstate * f.seqlen;
    ScanDetLayout l{(int64_t)f.batch, 0, 0, 0};
    if (fam == BwdFamily::generic) {
        l.nB = f.is_variable_B ? (cpg + kBwdGenR - 1) / kBwdGenR : f.batch;
        l.eB = f.is_variable_B ? bgnl : (int64_t)f.dim * f.dstate;
    } else if (fam == BwdFamily::tokens) {
        l.nA = (int64_t)f.batch * S;
        l.nB = ((cpg + kBwR - 1) / kBwR + W - 1) / W;
        l.eB = bgnl;
    } else {
        const int64_t cpb = (int64_t)W * (4 / (f.dstate / 16)) * kLsCPR, bpg = (cpg + cpb - 1) / cpb;
        l.nA = (int64_t)f.batch * S;
        l.nB = bpg > 2 ? bpg : 0;
        l.eB = bpg > 2 ? bgnl : 0;
    }
    l.bytes = sizeof(float) * (size_t)(l.nA * f.dim * (f.dstate + 2) + 2 * l.nB * l.eB);
    return l;
}

// The shape level does not know which family the call's pointers allow: the larger of the shape's family (at its
// segmentation; fewer segments only shrink it) and the generic fallback.
static size_t scan_bwd_det_workspace_bytes(const vivim_ssm_fwd_params& f) {
    BwdPlan q = plan_scan_bwd(f, nullptr);
    det_tokens_width(f, nullptr, q);
    const size_t gen = scan_det_layout(f, BwdFamily::generic, 1, 0).bytes;
    if (!q.W) return gen;
    const BwdFamily fam = q.K ? BwdFamily::tokens : BwdFamily::states;     // (the shape level sets K for lanes = tokens only)
    return std::max(gen, scan_det_layout(f, fam, q.S, q.W).bytes);
}

// The slots of the family this call's pointers select (never more than the shape-level size above).
static size_t scan_bwd_det_call_workspace_bytes(const vivim_ssm_bwd_params& p) {
    BwdPlan q = plan_scan_bwd(p.f, &p);
    if (q.family == BwdFamily::none) return 0;
    det_tokens_width(p.f, &p, q);
    return scan_det_layout(p.f, q.family, q.S, q.W).bytes;
}

// The deterministic protocol (det.cuh): a family that is not built and the slot workspace are refused before any launch.
static Launch ssm_bwd_det_dispatch(const vivim_ssm_bwd_params& p, void* det_ws, size_t det_ws_bytes, hipStream_t s) {
    const vivim_ssm_fwd_params& f = p.f;
    BwdPlan q = plan_scan_bwd(f, &p);
    if (q.family == BwdFamily::none) return Launch::unsupported;
    det_tokens_width(f, &p, q);
    const ScanDetLayout l = scan_det_layout(f, q.family, q.S, q.W);
    if (!det_ws_ok(det_ws, det_ws_bytes, l.bytes)) return Launch::bad_workspace;
    float* wA = static_cast<float*>(det_ws);
    float* wD = wA + l.nA * f.dim * f.dstate;
    float* wb = wD + l.nA * f.dim;
    float* wB = wb + l.nA * f.dim;
    float* wC = wB + l.nB * l.eB;
    vivim_ssm_bwd_params d = p;
    d.dA = wA; d.dA_d_stride = f.dstate; d.dA_dstate_stride = 1;
    if (p.dD) d.dD = wD;
    if (p.ddelta_bias) d.ddelta_bias = wb;
    const bool varBC = f.is_variable_B;
    if (l.nB) {
        d.dB = wB; d.dC = wC;
        if (varBC) {
            d.dB_batch_stride = d.dC_batch_stride = (int64_t)f.n_groups * f.dstate * f.seqlen;
            d.dB_group_stride = d.dC_group_stride = (int64_t)f.dstate * f.seqlen;
            d.dB_dstate_stride = d.dC_dstate_stride = f.seqlen;
        } else {                   // constant B / C: (dim, dstate), the channel on the group stride
            d.dB_batch_stride = d.dC_batch_stride = 0;
            d.dB_group_stride = d.dC_group_stride = f.dstate;
            d.dB_dstate_stride = d.dC_dstate_stride = 1;
        }
    }
    switch (q.family) {
        case BwdFamily::states: launch_ls_bwd(d, q, s, true); break;
        case BwdFamily::tokens: launch_bwd_fast(d, q, s, true); break;
        case BwdFamily::generic: launch_bwd_generic(d, q.ck, s, true); break;
        case BwdFamily::none: return Launch::unsupported;
    }
    det_reduce(wA, (int)l.nA, det_out(static_cast<float*>(p.dA), {f.dim, f.dstate}, {p.dA_d_stride, p.dA_dstate_stride}), s);
    if (p.dD) det_reduce(wD, (int)l.nA, det_out(static_cast<float*>(p.dD), {f.dim}, {1}), s);
    if (p.ddelta_bias) det_reduce(wb, (int)l.nA, det_out(static_cast<float*>(p.ddelta_bias), {f.dim}, {1}), s);
    if (l.nB) {
        auto bc = [&](float* w, void* out, int64_t bs, int64_t gs, int64_t ns) {
            if (varBC) det_reduce(w, (int)l.nB, det_out(static_cast<float*>(out), {f.batch, f.n_groups, f.dstate, f.seqlen}, {bs, gs, ns, 1}), s);
            else       det_reduce(w, (int)l.nB, det_out(static_cast<float*>(out), {f.dim, f.dstate}, {gs, ns}), s);
        };
        bc(wB, p.dB, p.dB_batch_stride, p.dB_group_stride, p.dB_dstate_stride);
        bc(wC, p.dC, p.dC_batch_stride, p.dC_group_stride, p.dC_dstate_stride);
    }
    return Launch::ok;
}

static bool ssm_bwd_dispatch(const vivim_ssm_bwd_params& p, hipStream_t s) {
    const BwdPlan q = plan_scan_bwd(p.f, &p);
    switch (q.family) {
        case BwdFamily::states: launch_ls_bwd(p, q, s); return true;
        case BwdFamily::tokens: launch_bwd_fast(p, q, s); return true;
        case BwdFamily::generic: launch_bwd_generic(p, q.ck, s); return true;
        case BwdFamily::none: break;
    }
    return false;
}

}  // namespace vivim

// ---- the C entry points.  The checks mirror the TORCH_CHECKs of the reference binding that still make sense below the
// tensor layer (selective_scan.cpp:233-304, 352-438).

// mode: the full forward, the backward (its `f` half), or the lean forward (no checkpoints; out_z alone when z is given)
enum SsmCheck { kSsmFwd, kSsmBwd, kSsmFwdLean };
static int check_ssm_fwd(const vivim_ssm_fwd_params* p, SsmCheck mode) {
    const bool is_bwd = mode == kSsmBwd;
    VCHECK(p != nullptr);
    VCHECK(dtype_ok(p->itype));
    VCHECK(p->batch > 0 && p->dim > 0 && p->seqlen > 0 && p->dstate > 0 && p->n_groups > 0);
    VCHECK(p->dstate <= 256);                       // selective_scan.cpp:262
    VCHECK(p->dim % p->n_groups == 0);
    VCHECK(p->u && p->delta && p->A && p->B && p->C);
    if (mode == kSsmFwdLean) {
        if (p->x != nullptr)
            return fail(VIVIM_ERR_INVALID, "selective_scan_fwd_lean: x must be NULL (this entry point writes no checkpoints; "
                        "vivim_selective_scan_fwd is the call that fills x)");
        if (p->z) {
            VCHECK(p->out_z != nullptr);
            if (p->out != nullptr)
                return fail(VIVIM_ERR_INVALID, "selective_scan_fwd_lean: with z only out_z is written, out must be NULL");
        } else {
            VCHECK(p->out != nullptr);
        }
    } else {
        VCHECK(p->x != nullptr || (is_bwd && p->seqlen <= vivim::scan_ckpt_len(*p)));
        if (!is_bwd) VCHECK(p->out != nullptr);
        if (p->z) {
            if (!is_bwd) VCHECK(p->out_z != nullptr);
            else VCHECK(p->out != nullptr);             // selective_scan.cpp:423 (saved out needed for dz)
        }
    }
    if (p->is_variable_B != p->is_variable_C)
        return fail(VIVIM_ERR_UNSUPPORTED,
                    "selective_scan: mixed constant/variable B and C is not built (Vivim uses variable B and C)");
    if (!p->is_variable_B) VCHECK(p->n_groups == 1);
    return VIVIM_OK;
}

static int check_ssm_bwd(const vivim_ssm_bwd_params* p) {
    VCHECK(p != nullptr);
    if (int rc = check_ssm_fwd(&p->f, kSsmBwd)) return rc;
    VCHECK(p->dout && p->du && p->ddelta && p->dA && p->dB && p->dC);
    VCHECK((p->f.D == nullptr) == (p->dD == nullptr));
    VCHECK((p->f.delta_bias == nullptr) == (p->ddelta_bias == nullptr));
    VCHECK((p->f.z == nullptr) == (p->dz == nullptr));
    return VIVIM_OK;
}

extern "C" {

int vivim_scan_chunk_len(int itype) { return vivim::scan_chunk_len(itype); }
int vivim_scan_ckpt_len(const vivim_ssm_fwd_params* f) { return f ? vivim::scan_ckpt_len(*f) : 0; }
size_t vivim_scan_bwd_workspace_bytes(const vivim_ssm_fwd_params* f) {
    return f ? vivim::scan_bwd_workspace_bytes(*f) : 0;
}
size_t vivim_scan_fwd_workspace_bytes(const vivim_ssm_fwd_params* f) {
    return f ? vivim::scan_fwd_workspace_bytes(*f) : 0;
}

int vivim_selective_scan_fwd(const vivim_ssm_fwd_params* p, void* stream) {
    if (int rc = check_ssm_fwd(p, kSsmFwd)) return rc;
    return after_dispatch(vivim::ssm_fwd_dispatch(*p, as_stream(stream)), "selective_scan_fwd",
                          "selective_scan_fwd not implemented for input type %d", p->itype);
}

int vivim_selective_scan_fwd_lean(const vivim_ssm_fwd_params* p, void* last_state, void* stream) {
    if (int rc = check_ssm_fwd(p, kSsmFwdLean)) return rc;
    return after_dispatch(vivim::ssm_fwd_lean_dispatch(*p, last_state, as_stream(stream)), "selective_scan_fwd_lean",
                          "selective_scan_fwd_lean not implemented for input type %d", p->itype);
}

int vivim_selective_scan_bwd(const vivim_ssm_bwd_params* p, void* stream) {
    if (int rc = check_ssm_bwd(p)) return rc;
    return after_dispatch(vivim::ssm_bwd_dispatch(*p, as_stream(stream)), "selective_scan_bwd",
                          "selective_scan_bwd not implemented for input type %d", p->f.itype);
}

size_t vivim_scan_bwd_det_workspace_bytes(const vivim_ssm_fwd_params* f) {
    return f && f->batch > 0 && f->dim > 0 && f->seqlen > 0 && f->dstate > 0 && f->n_groups > 0
               ? vivim::scan_bwd_det_workspace_bytes(*f) : 0;
}

size_t vivim_scan_bwd_det_call_workspace_bytes(const vivim_ssm_bwd_params* p) {
    return check_ssm_bwd(p) == VIVIM_OK ? vivim::scan_bwd_det_call_workspace_bytes(*p) : 0;
}

int vivim_selective_scan_bwd_det(const vivim_ssm_bwd_params* p, void* det_ws, size_t det_ws_bytes, void* stream) {
    if (int rc = check_ssm_bwd(p)) return rc;
    const size_t need = vivim::scan_bwd_det_call_workspace_bytes(*p);
    return after_det_dispatch(vivim::ssm_bwd_det_dispatch(*p, det_ws, det_ws_bytes, as_stream(stream)), "selective_scan_bwd_det",
                              "vivim_scan_bwd_det_call_workspace_bytes", det_ws, det_ws_bytes, need,
                              "selective_scan_bwd_det not implemented for input type %d", p->f.itype);
}

}  // extern "C"
