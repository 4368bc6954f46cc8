"""What an edge-conv layer of the encoder launches -- the gather kernel and its grid, how many table GEMMs, which side products -- is decided by
one pure host function (csrc/edge_plan.h).  Its paths agree to the bit or nearly, so no numerical test notices a changed choice; this one does:
the plan, compiled on its own with the host compiler, must name the kernel, the grid, the workgroup size and the number of table launches of every
case in tests/golden/edge_launches.json -- a kernel trace recorded from the library as it was before the layers' dispatch code became this
function (tests/tools/record_gemm_launches.py --family edge), in all three arithmetic modes.  No GPU needed."""
import importlib.util
import os
import subprocess
import sys

import pytest

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
TOOLS = os.path.join(REPO, "tests", "tools")
FIELDS = ("mode", "attn", "Cin", "Co", "head_c", "B", "Ns", "Nd", "has_rows", "fuse_q", "fuse_t", "want_rowmax", "want_colsum")
# one per EdgePlan enumerator (the table-free pair by its three launches' template arguments)
ENUMERATORS = ("ls::edge_pool_kernel", "ls::edge_pool_v4_kernel<8>", "ls::edge_pool_v4_kernel<16>", "ls::edge_attn_kernel", "ls::edge_attn_v4_kernel<16, 1>",
               "ls::edge_attn_v4_kernel<32, 1>", "ls::edge_attn_v4_kernel<64, 1>", "ls::edge_attn_v4_kernel<64, 2>", "ls::edge_attn_fq_kernel<16, 32>",
               "ls::edge_attn_fq_kernel<16, 64>", "ls::edge_attn_fq_kernel<32, 64>", "ls::edge_ft_v_kernel<128, 128, 1>", "ls::edge_ft_v_kernel<256, 32, 2>")


def _tool(name):
    if TOOLS not in sys.path:
        sys.path.insert(0, TOOLS)
    spec = importlib.util.spec_from_file_location(name, os.path.join(TOOLS, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def rec():
    return _tool("record_gemm_launches")


@pytest.fixture(scope="module")
def record(rec):
    return rec.load("edge")


def _compile(tmp, name):
    exe = str(tmp / name)
    subprocess.run([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(REPO, "livingscenes_amd", "csrc"),
                    os.path.join(TOOLS, name + ".cpp"), "-o", exe], check=True)
    return exe


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    """[EdgeTraits dict] -> [(launches [[name, grid, workgroup]] as the trace reports them, n_gemm, rowmax_parts, cs_rows)]"""
    exe = _compile(tmp_path_factory.mktemp("edge_plan"), "edge_plan_dump")

    def run(traits):
        lines = [" ".join(str(int(t[f])) for f in FIELDS) for t in traits]
        out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout.splitlines()
        assert len(out) == len(lines)
        res = []
        for line in out:
            launches, side = line.split(" # ")
            ls = [l.split("|") for l in launches.split(";")]
            res.append(([[n, [int(g) * int(b), 1, 1], [int(b), 1, 1]] for n, g, b in ls],) + tuple(int(v) for v in side.split()))
        return res
    run.exe = exe
    return run


@pytest.fixture(scope="module")
def vn_plan(tmp_path_factory):
    """[(mode, M, C, npts, a_parts)] -> the kernel name gemm_vn_plan gives the residual global conv ('none': GEMM + activation)"""
    exe = _compile(tmp_path_factory.mktemp("gemm_plan"), "gemm_plan_dump")

    def run(cases):
        # mode form M N K lda ldw pieces gather masked may_split latency has_planes wants_out_rowmax C npts has_G_or_cs a_parts has_a_rowmax has_w_rowmax
        lines = [f"{mode} 1 {M} 0 {C} {C} {C} 3 0 0 0 0 0 0 {C} {npts} 1 {parts} {int(parts > 0)} 1" for mode, M, C, npts, parts in cases]
        out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout.splitlines()
        return [l.split("|")[0] for l in out]
    return run


def test_the_record_lists_the_ladder(rec, record):
    want = {f"{mode}:{key}" for mode in rec.MODES for key, _, _ in rec.cases_of(mode, "edge")}
    assert want == set(record), "the ladder and the record list different cases: re-record (see the recorder's docstring)"
    assert all(v["sha256"] for v in record.values()), "two recordings from the library before the plan agreed on every case: every output is hashed"


def test_the_plan_names_every_recorded_export_launch(rec, record, plan):
    keys, traits = [], []
    for mode in rec.MODES:
        for key, model, op, (i, B, Ns, Nd, rows), opt in (c for c in rec.edge_ladder() if c[2] == "edgeconv"):
            keys.append(f"{mode}:{key}")
            traits.append(rec.edge_traits(rec.model_cfgs(model)[0], mode, i, B, Ns, Nd, rows, opt["OPT_EDGE_FUSE_Q"], opt["OPT_EDGE_FUSE_T"]))
    planned = dict(zip(keys, plan(traits)))
    wrong = {k: (planned[k], record[k]) for k in keys
             if planned[k][0] != [l[:3] for l in record[k]["launches"]] or planned[k][1] != record[k]["tables"] or planned[k][2:] != (0, 0)}
    assert not wrong, f"{len(wrong)} of {len(keys)} cases: the plan differs from the recorded launches (planned, recorded): {dict(list(wrong.items())[:4])}"
    # every enumerator and every arithmetic mode is in the comparison
    names = {l[0] for k in keys for l in record[k]["launches"]}
    assert not set(ENUMERATORS) - names, set(ENUMERATORS) - names
    assert {k.split(":", 1)[0] for k in keys} == set(rec.MODES)
    assert {record[k]["tables"] for k in keys} == {0, 1, 2}


def _mean_launch(B, Co, Nd, cs_rows, vn_kernel):
    """The mean launch of the residual global conv (model.hip: global_conv; pointwise.hip: glob_mean_gemv_launch, mean_points_launch) as the
    trace reports it, or None: the streaming kernel finishes the mean from the producer's column sums itself."""
    if vn_kernel == "none":
        return ["ls::mean_points_kernel", [-(-3 * Co // 64) * 256, B, 1], [256, 1, 1]]
    if 0 < cs_rows <= 32 and vn_kernel.startswith("ls::gemm_vn_direct_kernel"):
        return None
    ncols, nblk = 2 * Co, 1
    wg_cap, min_cols = (2048, 32) if cs_rows > 0 else (512, 64)
    while B * nblk < wg_cap and ncols // (nblk * 2) >= min_cols:
        nblk *= 2
    cpb = -(-ncols // nblk)
    return ["ls::glob_mean_gemv_kernel", [B * 256, -(-ncols // cpb), 1], [256, 1, 1]]


def test_the_plan_names_every_recorded_encode_launch(rec, record, plan, vn_plan):
    rwb = _tool("record_workspace_bytes")
    ecfg = rec.model_cfgs("released")[0]
    fd, g0 = ecfg["feat_dim"], ecfg["res_global_start_layer"]
    seen, cs_seen = set(), set()
    for mode in rec.MODES:
        for key, _, _, (B, N), _ in (c for c in rec.edge_ladder() if c[2] == "encode"):
            sizes = rwb.layer_sizes(ecfg, N)
            planned = plan([rec.edge_traits(ecfg, mode, i, B, Ns, Nd, rows, encode=True) for i, (Ns, Nd, rows) in enumerate(sizes) if i >= 1])
            vn = vn_plan([(rec.MODES.index(mode), B * sizes[i][1] * 3, fd[i], sizes[i][1], planned[i - 1][2]) for i in range(max(g0, 1), len(sizes))])
            want = [["ls::edge_l0_kernel", [-(-B * N // 8) * 256, 1, 1], [256, 1, 1]]]
            for i, (launches, _, _, cs_rows) in enumerate(planned, 1):
                want += launches
                if i >= g0:
                    mean = _mean_launch(B, fd[i], sizes[i][1], cs_rows, vn[i - max(g0, 1)])
                    want += [mean] if mean else []
                    cs_seen.add((i, cs_rows > 0))
            got = [l[:3] for l in record[f"{mode}:{key}"]["launches"]]
            assert sorted(want) == got, (mode, key, sorted(want), got)
            seen |= {l[0] for l in got}
    # table-free and fused layers, both mean kernels, and layers with and without column sums are in the comparison
    for name in ("ls::edge_ft_v_kernel<128, 128, 1>", "ls::edge_ft_v_kernel<256, 32, 2>", "ls::edge_attn_fq_kernel<32, 64>", "ls::edge_attn_v4_kernel<64, 2>",
                 "ls::glob_mean_gemv_kernel", "ls::mean_points_kernel"):
        assert name in seen, name
    assert {(5, True), (5, False), (6, True), (6, False), (2, True), (2, False)} <= cs_seen


def test_the_32_bit_offset_limits_by_their_arithmetic(plan):
    """edge_off32_fits: no handle reaches these sides (a 4 GB neighbour-side table, 2^24 source rows in a batch, 2^24 bytes per point, 65536 source
    points), so no launch is recorded there.  They are conditions: just inside fits, just outside does not, each limit on its own."""
    out = subprocess.run([plan.exe], input="limits\n", capture_output=True, text=True, check=True).stdout.split()
    assert out == ["10", "10", "10", "10"], out
    assert 65535 * 12 * 5461 < 2 ** 32 <= 65535 * 12 * 5462 and 16384 * 1024 == 2 ** 24 and 12 * 1398101 < 2 ** 24 <= 12 * 1398102
    # ... and they decide: a fused layer and a float4 pool layer one source point below / at 65536 (the other limits far away)
    ok, over = 65535, 65536
    t = lambda attn, Ns: dict(mode=0, attn=attn, Cin=32, Co=64 if attn else 32, head_c=16, B=1, Ns=Ns, Nd=64, has_rows=1, fuse_q=1, fuse_t=1, want_rowmax=0,
                              want_colsum=0)
    res = plan([t(1, ok), t(1, over), t(0, ok), t(0, over)])
    assert [r[0][0][0] for r in res] == ["ls::edge_attn_fq_kernel<16, 32>", "ls::edge_attn_v4_kernel<16, 1>", "ls::edge_pool_v4_kernel<8>", "ls::edge_pool_kernel"]
    assert [r[1] for r in res] == [1, 2, 2, 2]


def test_the_float64_ladder_reaches_every_enumerator(plan):
    """tests/tools/edge_vs_float64.py: the cases tests/test_hip_edge_layers_f64.py holds to the float64 layer oracle.  In the default mode the
    kernels the plan names for them are all thirteen ENUMERATORS; under bf16x3 and fp32 every case plans a table kernel (a table GEMM or two,
    none of the fused or table-free forms).  This keeps the ladder honest when the plan changes.  The one branch no case takes is
    edge_off32_fits() == false: it needs a table of 4 GB or more (test_the_32_bit_offset_limits_by_their_arithmetic holds it by its arithmetic)."""
    lad = _tool("edge_vs_float64")
    cases = [c for c in lad.ladder() if c[2] >= 1]
    assert len(cases) > 60 and {c[2] for c in lad.ladder()} == set(range(7))
    names = {r[0][-1][0] for r in plan([lad.traits(c, lad.MODES[0]) for c in cases])}
    assert names == set(ENUMERATORS), (names - set(ENUMERATORS), set(ENUMERATORS) - names)
    fused = tuple(n for n in ENUMERATORS if "_fq_" in n or "_ft_" in n)
    for mode in lad.MODES[1:]:
        res = plan([lad.traits(c, mode) for c in cases])
        wrong = [c[0] for c, r in zip(cases, res) if r[1] not in (1, 2) or r[1] != 1 + c[3][3] or r[0][-1][0] in fused or len(r[0]) != 1]
        assert not wrong, (mode, wrong[:4])


def test_the_reduced_schedules_plan_the_kernels_with_side_products(rec, plan):
    """The encodes of tests/test_hip_edge_layers_f64.py (edge_vs_float64.reduced_cfg): what their layers >= 2 launch inside ls_encode, and
    whether row maxima and column sums are written."""
    lad, rwb = _tool("edge_vs_float64"), _tool("record_workspace_bytes")
    got = {}
    for name, N in lad.REDUCED:
        cfg = lad.reduced_cfg(name)
        sizes = rwb.layer_sizes(cfg, N)
        for fq in (1, 0):
            res = plan([rec.edge_traits(cfg, "f16", i, 3, *sizes[i], fuse_q=fq, encode=True) for i in range(1, cfg["num_layers"])])
            got[(name, N, fq)] = [(r[0][-1][0].replace("ls::edge_", "").replace("_kernel", ""), r[2] > 0, r[3] > 0) for r in res]
    for fq in (1, 0):
        assert got[("ft256", 32, fq)] == [("pool", False, False), ("ft_v<256, 32, 2>", True, True)]
        assert got[("ft128", 128, fq)] == [("pool", False, False), ("ft_v<128, 128, 1>", True, True)]
    for N, cs in ((64, True), (72, False)):
        assert got[("fq", N, 1)] == [("pool_v4<8>", False, False)] + [(f"attn_fq<{k}>", True, cs) for k in ("16, 32", "16, 64", "32, 64")]
        assert got[("fq", N, 0)] == [("pool_v4<8>", False, False)] + [(f"attn_v4<{k}, 1>", True, cs) for k in (16, 16, 32)]
