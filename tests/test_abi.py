"""CPU: the C-ABI shared library loads without a GPU, exports every symbol include/vivim_hip.h declares,
agrees with the ctypes struct layouts, and rejects bad params before any launch."""
import ctypes
import os
import re

import pytest

from conftest import ROOT
from vivim_amd import _lib


def _declared_functions():
    text = open(os.path.join(ROOT, "include", "vivim_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(vivim_[a-z0-9_]+)\s*\(", text)))


def test_header_symbols_exported():
    L = _lib.lib()
    names = _declared_functions()
    assert set(_lib.EXPORTS) == set(names)
    for n in names:
        assert hasattr(L, n), n


def test_struct_layouts_match():
    L = _lib.lib()
    for which, st in enumerate((_lib.SsmFwdParams, _lib.SsmBwdParams, _lib.ConvFwdParams, _lib.ConvBwdParams,
                                _lib.DwConvParams, _lib.DwConvWgradParams, _lib.DirParams, _lib.ConvUpdateParams,
                                _lib.StateUpdateParams, _lib.LayerNormParams, _lib.WgradNtParams)):
        assert L.vivim_sizeof(which) == ctypes.sizeof(st)
    assert L.vivim_sizeof(99) == 0
    assert L.vivim_abi_version() == 8
    assert L.vivim_scan_chunk_len(_lib.F32) > 0 and L.vivim_scan_chunk_len(_lib.BF16) % 64 == 0


def test_checkpoint_length_is_a_function_of_shape_and_tuning():
    """vivim_scan_ckpt_len: short rows (16 tokens per dstate-16 row) for the shapes the lanes=states backward is chosen for,
    the long rows otherwise; forward tuning 1-3 (families that write long rows) and 5 / 6 (short rows) override the choice."""
    L = _lib.lib()
    s = _lib.SsmFwdParams()
    s.batch, s.dim, s.n_groups, s.dstate, s.seqlen, s.itype = 2, 64, 1, 16, 1280, _lib.BF16
    s.is_variable_B = s.is_variable_C = 1
    s.u_d_stride = s.delta_d_stride = s.B_dstate_stride = s.C_dstate_stride = 1280
    long_rows = L.vivim_scan_chunk_len(_lib.BF16)
    prev = L.vivim_set_tuning(0, 0)
    try:
        assert L.vivim_scan_ckpt_len(ctypes.byref(s)) == 16
        s.seqlen = 20480                                  # 16-bit rows up to 32768 tokens: still the lanes=states backward (round 3)
        s.u_d_stride = s.delta_d_stride = s.B_dstate_stride = s.C_dstate_stride = 20480
        assert L.vivim_scan_ckpt_len(ctypes.byref(s)) == 16
        s.itype = _lib.F32                                # fp32 rows longer than 8192: the lanes=tokens backward, long checkpoint rows
        assert L.vivim_scan_ckpt_len(ctypes.byref(s)) == L.vivim_scan_chunk_len(_lib.F32)
        s.itype = _lib.BF16
        s.seqlen = 40960
        s.u_d_stride = s.delta_d_stride = s.B_dstate_stride = s.C_dstate_stride = 40960
        assert L.vivim_scan_ckpt_len(ctypes.byref(s)) == long_rows
        L.vivim_set_tuning(0, 6)
        assert L.vivim_scan_ckpt_len(ctypes.byref(s)) == 16
        s.dstate = 64
        assert L.vivim_scan_ckpt_len(ctypes.byref(s)) == 64
        s.dstate = 24                                     # not a whole number of 16-lane rows
        assert L.vivim_scan_ckpt_len(ctypes.byref(s)) == long_rows
        s.dstate = 16
        L.vivim_set_tuning(0, 1)
        assert L.vivim_scan_ckpt_len(ctypes.byref(s)) == long_rows
        s.is_variable_B = s.is_variable_C = 0
        L.vivim_set_tuning(0, 0)
        assert L.vivim_scan_ckpt_len(ctypes.byref(s)) == long_rows
    finally:
        L.vivim_set_tuning(0, prev)


def test_scan_plan_queries_pinned():
    """vivim_scan_ckpt_len / vivim_scan_*_workspace_bytes for one shape per forward family and for the backward families,
    as literals.  None of them depends on an occupancy query (those differ between a build host and the GPU)."""
    L = _lib.lib()

    def query(itype, batch, dim, groups, dstate, seqlen, variable=1):
        s = _lib.SsmFwdParams()
        s.batch, s.dim, s.n_groups, s.dstate, s.seqlen, s.itype = batch, dim, groups, dstate, seqlen, itype
        s.is_variable_B = s.is_variable_C = variable
        s.u_d_stride = s.delta_d_stride = s.out_d_stride = s.B_dstate_stride = s.C_dstate_stride = seqlen
        s.u_batch_stride = s.delta_batch_stride = s.out_batch_stride = seqlen * dim
        s.B_group_stride = s.C_group_stride = seqlen * dstate
        s.B_batch_stride = s.C_batch_stride = seqlen * dstate * groups
        return (L.vivim_scan_ckpt_len(ctypes.byref(s)), L.vivim_scan_fwd_workspace_bytes(ctypes.byref(s)),
                L.vivim_scan_bwd_workspace_bytes(ctypes.byref(s)))

    prev = (L.vivim_set_tuning(0, 0), L.vivim_set_tuning(1, 0))
    try:
        # lanes = channels forward (fp32 B / C copy + segment carries), lanes = tokens backward (8 segments)
        assert query(_lib.BF16, 2, 768, 3, 16, 40960) == (256, 39813888, 1622016)
        assert query(_lib.F16, 2, 768, 3, 64, 8192) == (256, 50727936, 6340608)
        assert query(_lib.BF16, 2, 768, 3, 24, 5124)[:2] == (256, 0)                     # n-split forward: no workspace
        assert query(_lib.F32, 2, 64, 1, 16, 1280, variable=0) == (256, 0, 0)           # generic kernels
        ck, fwd_ws, _ = query(_lib.BF16, 2, 64, 1, 16, 1280)                              # lanes = states forward, 20 segments
        assert (ck, fwd_ws) == (16, 337920)
        # lanes = states backward: whole (batch, dim, segment) records of 2 * dstate + 1 floats; none when unsegmented
        unit = 2 * 768 * (2 * 16 + 1) * 4
        for seqlen in (320, 1280, 20480):
            ck, _, bwd_ws = query(_lib.BF16, 2, 768, 3, 16, seqlen)
            assert ck == 16 and bwd_ws % unit == 0 and bwd_ws // unit >= 2
        assert query(_lib.BF16, 2, 768, 3, 16, 64)[2] == 0                                 # four checkpoint blocks: one segment
    finally:
        L.vivim_set_tuning(0, prev[0])
        L.vivim_set_tuning(1, prev[1])


def test_rejects_before_launch():
    """Invalid params are refused on the host (no GPU needed): null struct, bad width, bad dtype."""
    L = _lib.lib()
    assert L.vivim_selective_scan_fwd(None, None) == 1
    assert b"check failed" in L.vivim_last_error()
    p = _lib.ConvFwdParams()
    p.batch, p.dim, p.seqlen, p.width = 1, 4, 8, 5
    p.x, p.weight, p.out = 1, 1, 1
    p.x_l_stride = p.out_l_stride = 1
    assert L.vivim_causal_conv1d_fwd(ctypes.byref(p), None) == 1
    assert b"width between 2 and 4" in L.vivim_last_error()
    p.width, p.itype = 4, 7
    assert L.vivim_causal_conv1d_fwd(ctypes.byref(p), None) == 1
    p.itype, p.x_l_stride, p.x_c_stride = 0, 4, 2
    assert L.vivim_causal_conv1d_fwd(ctypes.byref(p), None) == 1          # neither seqlen nor channels contiguous
    assert b"unit stride along seqlen or along channels" in L.vivim_last_error()
    p.x_c_stride = 1                                                      # channel-last x needs a channel-last out
    assert L.vivim_causal_conv1d_fwd(ctypes.byref(p), None) == 1
    s = _lib.SsmFwdParams()
    s.batch = s.dim = s.seqlen = s.n_groups = 1
    s.dstate = 300
    assert L.vivim_selective_scan_fwd(ctypes.byref(s), None) == 1


def test_call_raises_runtime_error():
    with pytest.raises(RuntimeError, match="check failed"):
        _lib.call("vivim_selective_scan_fwd", _lib.SsmFwdParams(), 0)


def test_python_surface_imports_without_gpu():
    import causal_conv1d  # noqa: F401
    import causal_conv1d_cuda
    import mamba_ssm
    import selective_scan_cuda
    from modeling.vivim import MambaLayer, Vivim, mamba_block  # noqa: F401
    assert callable(selective_scan_cuda.fwd) and callable(selective_scan_cuda.bwd)
    assert callable(causal_conv1d_cuda.causal_conv1d_fwd) and callable(causal_conv1d_cuda.causal_conv1d_bwd)
    assert hasattr(mamba_ssm, "Mamba") and hasattr(mamba_ssm, "selective_scan_fn")


def test_product_never_imports_oracle():
    """The oracle is test infrastructure: nothing under vivim_amd/ (or the alias packages) may reference it."""
    bad = []
    for top in ("vivim_amd", "mamba_ssm", "causal_conv1d", "modeling"):
        for dp, _, files in os.walk(os.path.join(ROOT, top)):
            for f in files:
                if f.endswith((".py", ".hip", ".cuh", ".h")):
                    src = open(os.path.join(dp, f)).read()
                    if re.search(r"^\s*(from|import)\s+oracle\b|ssm_oracle|ref_torch", src, flags=re.M):
                        bad.append(os.path.join(dp, f))
    assert not bad, bad


def test_tuning_roundtrip():
    """vivim_set_tuning returns the previous value and rejects bad arguments (no GPU needed)."""
    L = _lib.lib()
    prev = L.vivim_set_tuning(0, 5)
    assert prev >= 0
    assert L.vivim_set_tuning(0, prev) == 5
    assert L.vivim_set_tuning(2, 0) == -1 and L.vivim_set_tuning(0, -3) == -1


def test_dir_maps_reject_bad_arguments_on_host():
    """vivim_dir_scatter / vivim_dir_gather validate before launching (no GPU needed for the rejections)."""
    import ctypes
    L = _lib.lib()
    P = _lib.DirParams()
    P.batch, P.channels, P.seqlen, P.nframes, P.csplit, P.itype, P.scale = 1, 4, 30, 5, 2, _lib.BF16, 1.0
    P.src = P.dst = 0
    for fn in (L.vivim_dir_scatter, L.vivim_dir_gather):
        assert fn(ctypes.byref(P), None) != 0                      # null pointers
    P.src = P.dst = 4096
    assert L.vivim_dir_scatter(ctypes.byref(P), None) != 0        # 30 bf16 tokens are not whole 16-byte vectors
    P.seqlen, P.nframes = 32, 5
    assert L.vivim_dir_scatter(ctypes.byref(P), None) != 0        # seqlen not a multiple of nframes
    assert b"" != L.vivim_last_error()


def test_graft_entry_build_is_consistent():
    """__graft_entry__.build() (what the driver runs every round) must accept the library it has just built: its ABI
    assertion is derived from the header, not hard-coded."""
    import __graft_entry__ as g
    g.build()


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as fh:
        return fh.read()


def test_no_experiment_scaffolding_in_kernel_sources():
    """Timing-ablation switches (FOO_ABL) and in-kernel stamp hooks (VIVIM_STAMP*) are retired: the product build is the
    only build of the kernel sources."""
    bad = []
    for top in (os.path.join("vivim_amd", "csrc"), "include"):
        for dp, _, files in os.walk(os.path.join(ROOT, top)):
            for f in files:
                if f.endswith((".hip", ".cuh", ".h", ".hpp", ".cpp")) or f == "Makefile":
                    src = open(os.path.join(dp, f)).read()
                    bad += ["%s: %s" % (f, m) for m in re.findall(r"\b[A-Z0-9]+_ABL\b|VIVIM_STAMP", src)]
    assert not bad, bad


def test_env_switches_match_integration_table():
    """The VIVIM_* variables the library, its Python wrappers and bench.py read are exactly the rows of INTEGRATION.md §4."""
    read = set()
    csrc = os.path.join(ROOT, "vivim_amd", "csrc")
    for f in sorted(os.listdir(csrc)):
        if f.endswith((".hip", ".cuh", ".h")):
            src = _read("vivim_amd", "csrc", f)
            read |= set(re.findall(r'\b(?:getenv|num)\(\s*"(VIVIM_\w+)"', src))
            read |= set(re.findall(r'\btuning_get\([^,()]*,\s*"(VIVIM_\w+)"', src))
    py = [os.path.join("vivim_amd", f) for f in sorted(os.listdir(os.path.join(ROOT, "vivim_amd"))) if f.endswith(".py")]
    for f in py + ["bench.py"]:
        src = _read(f)
        for m in re.findall(r'os\.(?:environ\.get|getenv)\(\s*["\'](VIVIM_\w+)|os\.environ\[\s*["\'](VIVIM_\w+)|'
                            r'["\'](VIVIM_\w+)["\']\s+(?:not\s+)?in\s+os\.environ', src):
            read |= {n for n in m if n}
    doc = _read("INTEGRATION.md")
    section = re.search(r"^## 4\..*?$(.*?)^## ", doc, flags=re.S | re.M).group(1)
    documented = set()
    for line in section.splitlines():
        if line.startswith("| `"):
            documented |= set(re.findall(r"`(VIVIM_\w+)", line.split("|")[1]))
    assert read, "no environment reads found: the patterns above no longer match the code"
    assert read == documented, {"read but not in INTEGRATION.md §4": sorted(read - documented),
                                "in INTEGRATION.md §4 but not read": sorted(documented - read)}
