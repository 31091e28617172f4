// scan_plan.cuh -- host-side plan of the selective-scan launches (scan_plan.hip) and what the kernel files share with it.
//
// A plan has two levels.  The SHAPE level reads sizes, strides, flags and the tuning values, never pointers: it alone
// decides the checkpoint length of `x` and the workspace sizes, so the forward call, the backward call and the allocation
// of `x` agree by construction.  The LAUNCH level adds what pointers decide (16-byte vector rows, a workspace that is
// present and large enough) and picks the family that runs.  The family files only issue the launches of their plan.
#pragma once
#include <initializer_list>
#include "ls_common.cuh"
#include "det.cuh"

namespace vivim {

// Tuning values (vivim_set_tuning, VIVIM_FWD_VARIANT / VIVIM_BWD_VARIANT): ABI, the numbers must not change.
enum FwdTune { kFwdAuto = 0, kFwdNsplitK8 = 1, kFwdNsplitK4 = 2, kFwdGeneric = 3, kFwdChan = 5, kFwdStates = 6 };
enum BwdTune { kBwdAuto = 0, kBwdTokensW8 = 1, kBwdTokensW4 = 2, kBwdGeneric = 3, kBwdStates1 = 4, kBwdStates2 = 5 };

enum class FwdFamily { none, nsplit, generic, chan, states };
enum class BwdFamily { none, tokens, generic, states };

constexpr int kNsR = 2;            // n-split forward: channels per workgroup
constexpr int kChWaves = 2;        // lanes = channels forward: independent waves per workgroup
constexpr int kBwWmax = 8;         // lanes = tokens backward: waves per workgroup, 8 or 4 (template parameter W of the fast kernel)
constexpr int kBwR = 2;            // lanes = tokens backward: channels per wave
constexpr int kBwdGenR = 2;        // generic backward: channels per wave

// Lanes = channels forward, tokens per tile: a tile row is ONE 128-byte line for every I/O type (32 fp32 / 64 16-bit tokens).
// With 32-byte pieces (16 tokens of bf16, the first version) a line of a row was fetched for four separate tiles,
// microseconds apart, with 2048 waves x 64 rows x 3 streams of such lines in flight -- far more than the L2s hold:
// rocprofv3 counted 1.17 GB of HBM traffic per launch against 0.25 GB algorithmic at cfg 2's grouped stage 0 (4.1 TB/s in
// 283 us) and 4.6 GB against 1.76 GB at cfg 3's stage 0 (4.8 TB/s in 962 us): the launches were bound by their own
// over-fetch (profiles/r02_hbm_counters_per_kernel.txt).  Whole lines need 18 KB of LDS per wave for TWO resident streams,
// which is what 8 waves per CU can have: z no longer goes through LDS -- the gate out * silu(z) is applied in the store
// phase, where the lanes lie along tokens again and z is read with the same coalesced vectors the outputs are written
// with; y waits for it in LDS as fp32, in the bytes of the u / delta tokens it was computed from.
template <typename T> struct ChTile { static constexpr int TT = 128 / (int)sizeof(T); };

struct FwdPlan {
    FwdFamily family;
    int ck;                        // tokens per checkpoint row of x
    int S, seg;                    // token-axis segments (1: none) and their length (chan: tiles, states: checkpoint blocks)
    size_t ws;                     // workspace bytes the shape asks for (the larger of the two families that may run)
    int K;                         // n-split: tokens per lane (8 or 4)
    int Lpad, xcd;                 // lanes = channels: padded row length of the fp32 B / C copy, XCD re-numbering
    size_t bc_floats;              // lanes = channels: floats of that copy (the segment carries follow it)
    bool bc_vec;                   // lanes = states: B / C rows read with 16-byte vectors
};

struct BwdPlan {
    BwdFamily family;
    int ck;                        // tokens per checkpoint row of x (as the forward wrote it)
    int S, seg;                    // token-axis segments (1: none) and their length (tokens: steps, states: checkpoint blocks)
    size_t ws;                     // workspace bytes the shape asks for
    int K, W;                      // lanes = tokens: tokens per lane, waves per workgroup; lanes = states: waves per workgroup
    bool da_lds;                   // lanes = tokens: per-lane dA partials in LDS
    bool ls2;                      // lanes = states: second-generation main kernel (scan_ls2.hip)
    bool closed_prepass;           // lanes = states: the lanes = tokens closed-form pre-pass + carry (scan_bwd.hip)
    bool bc_vec;                   // lanes = states: B / C rows read with 16-byte vectors
};

// Environment knobs of the planner and the family files (sweeps and diagnostics), read once.
struct ScanEnv {
    int chan_waves;                // VIVIM_CHAN_WAVES: target waves of the lanes = channels segmentation
    int chan_xcd;                  // VIVIM_CHAN_XCD: force the XCD re-numbering on (1) / off (0)
};
const ScanEnv& scan_env();

// Every hipFuncSetAttribute a dynamic-LDS launch above 64 KB needs (a host-side table write, no synchronisation).
template <typename K> inline void allow_smem(K kernel, size_t smem) {
    if (smem > 65536)
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
}
// Resident workgroups per CU from the occupancy query; `fallback` where there is no device to ask (a build host).
template <typename K> inline int occupancy_query(K kernel, int W, size_t smem, int fallback) {
    int nb = 0;
    allow_smem(kernel, smem);
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, kernel, W * kWave, smem) != hipSuccess || nb <= 0) {
        (void)hipGetLastError();
        nb = fallback;
    }
    return nb;
}

// Family launches (kernel files).  Each issues exactly the launches of its plan.
// `lean`: the variant of the output pass without checkpoint stores (and without the `out` store when z is given); the
// params' `x` is then null or the (batch, dim, dstate) fp32 buffer that receives the state after the last token.
void launch_fwd_nsplit(const vivim_ssm_fwd_params&, const FwdPlan&, hipStream_t, bool lean = false);   // scan_fwd.hip
void launch_fwd_generic(const vivim_ssm_fwd_params&, hipStream_t, bool lean = false);
void launch_fwd_chan(const vivim_ssm_fwd_params&, const FwdPlan&, hipStream_t, bool lean = false);     // scan_fwd_chan.hip
void launch_ls_fwd(const vivim_ssm_fwd_params&, const FwdPlan&, hipStream_t, bool lean = false);       // scan_ls.hip
// `det`: the deterministic variant (scan_det_layout in scan_plan.hip), with p's reduced outputs pointing into the slot workspace.
void launch_ls_bwd(const vivim_ssm_bwd_params&, const BwdPlan&, hipStream_t, bool det = false);
void launch_ls2_bwd(const vivim_ssm_bwd_params&, const LsSeg&, int W, hipStream_t, bool det = false);   // scan_ls2.hip
void launch_bwd_fast(const vivim_ssm_bwd_params&, const BwdPlan&, hipStream_t, bool det = false);       // scan_bwd.hip
void launch_bwd_generic(const vivim_ssm_bwd_params&, int ck, hipStream_t, bool det = false);
void launch_bwd_closed_prepass(const vivim_ssm_bwd_params&, const LsSeg&, int K, hipStream_t);
// Raw occupancy of the lanes = states backward main kernel `f` selects (first / second generation); cached by the planner.
int ls_bwd_occupancy(const vivim_ssm_fwd_params& f, int W);                            // scan_ls.hip
int ls2_bwd_occupancy(const vivim_ssm_fwd_params& f, int W);                           // scan_ls2.hip

}  // namespace vivim
