"""The split-precision rows GEMMs keep their prefetch in flight across the MFMAs (host only: reads
the gfx950 code objects of libunet_hip.so through tools/kloop_waits.py, no GPU).

gemm_rows_vec loads stage k+1 into registers before the MFMAs of stage k and consumes it after them
(DESIGN.md §4).  The source said so before the generated code did: with the loads under
`if (kt + 1 < nk)` the staged registers were loop-carried, and the compiler's copies into the carried
set sat right behind the loads, under `s_waitcnt vmcnt` counts that waited for up to eight of the
fourteen loads just issued.  Condition held here, for the ten `gemm_rows_vec<128, 128, 32, ..., true>`
kernels of launch_rows' (operand mode, dropout, epilogue) triples: inside the k-loop, between the first
load of a run of loads and the next v_mfma, no s_waitcnt asks for a vmcnt below the number of
vector-memory operations issued since that first load."""
import importlib.util
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]


def _tool_module():
    spec = importlib.util.spec_from_file_location("kloop_waits", ROOT / "tools" / "kloop_waits.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


K = _tool_module()

# kernels the compiler leaves with a wait that cannot be removed without spills: none today
EXCLUDED = {}


@pytest.fixture(scope="module")
def x6_rows():
    if not (K.LIB.exists() and K.tool("llvm-objcopy") and K.tool("llvm-objdump")):
        pytest.skip("needs the built libunet_hip.so and llvm-objcopy / llvm-objdump")
    return K.table(K.LIB, K.X6_ROWS)


def test_every_x6_rows_kernel_is_found(x6_rows):
    # BM, BN, BK = 128, 128, 32; (AMODE, DROP, EPI) = launch_rows' ten triples; BKC and X6 true
    triples = {(0, 0, 0), (0, 0, 1), (3, 0, 0), (3, 1, 0), (0, 0, 2), (0, 1, 2), (1, 0, 2), (1, 1, 2), (2, 0, 0), (2, 0, 3)}
    want = {f"ILi128ELi128ELi32ELi{a}ELb{d}ELi{e}ELb1ELb1EEEv" for a, d, e in triples}
    got = {w for w in want if any(w in name for name in x6_rows)}
    assert got == want, sorted(want - got)
    assert len(x6_rows) == 10, sorted(x6_rows)


def test_prefetch_stays_in_flight_across_the_mfmas(x6_rows):
    bad = {}
    for name, runs in x6_rows.items():
        if name in EXCLUDED:
            continue
        assert runs, f"{name}: no load run in front of the k-loop's MFMAs"
        # the whole stage is issued in front of the MFMAs: 4 A quads (+ 4 z, + 2 coefficient vectors) and 6 B chunks
        assert sum(r["loads"] for r in runs) >= 10, (name, runs)
        if any(r["drained"] > 0 for r in runs):
            bad[name] = runs
    assert not bad, bad


def test_the_tool_sees_a_drained_prefetch():
    # a listing in the compiler's form: four loads, then a wait that leaves two outstanding, then the MFMA
    asm = "\n".join(["_Zkernel:", ".LBB0_1:",
                     "\tglobal_load_dwordx4 v[0:3], v[40:41], off", "\tglobal_load_dwordx4 v[4:7], v[42:43], off",
                     "\tglobal_load_dwordx4 v[8:11], v[44:45], off", "\tglobal_load_dwordx4 v[12:15], v[46:47], off",
                     "\ts_waitcnt vmcnt(2)", "\tv_mov_b32_e32 v20, v0",
                     "\tv_mfma_f32_32x32x16_bf16 a[0:15], v[24:27], v[28:31], a[0:15]",
                     "\ts_waitcnt vmcnt(0)", "\tds_write_b128 v50, v[0:3]", "\ts_barrier",
                     "\ts_cbranch_scc0 .LBB0_1", "\ts_endpgm", ".Lfunc_end0:"])
    code = K.parse_asm(asm, lambda s: True)["_Zkernel"]
    assert K.runs(code) == [{"loads": 4, "minwait": 2, "drained": 2}]
    healthy = asm.replace("\ts_waitcnt vmcnt(2)\n\tv_mov_b32_e32 v20, v0\n", "")
    assert K.runs(K.parse_asm(healthy, lambda s: True)["_Zkernel"]) == [{"loads": 4, "minwait": None, "drained": 0}]
