"""Host side of the count tree in global memory (``rnampnn_design_count_long`` / ``rnampnn_design_count_profile_long``,
csrc/design_long.hip): the workspace sizes against the header's formula, every argument error before a launch (so no GPU is needed), the
limits, the ``tree=`` keyword's refusals in the decode functions, the models and predict.py, ``tree="lds"`` keeping today's message, and the
margins of the restatement's draws of the device tests' long cases (tests/_design_long_case.py), which is why no draw is left out there."""
import ctypes as C
import os
import re
import sys

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "rna-mpnn_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _design_long_case as L  # noqa: E402

T_MAX_WALK = 32744                                                 # the largest T whose walk fits 160 KiB of LDS (include/rnampnn_hip.h)


@pytest.fixture(scope="module")
def native():
    import __graft_entry__ as g
    g.build()
    from rnampnn import _native
    return _native


# ---------------------------------------------------------------------------------------------------------------- the workspace
@pytest.mark.parametrize("T, cap", [(1, 1), (2, 2), (1017, 1017), (1018, 1018), (4417, 8), (8192, 8192)])
def test_workspace_bytes_are_the_headers_formula(native, T, cap):
    lib = native.lib()
    for B in (1, 3):
        assert lib.rnampnn_design_count_long_workspace_bytes(B, T, cap) == 8 * B * L.tree_doubles(T, cap)
        assert lib.rnampnn_design_count_profile_long_workspace_bytes(B, T, cap) == 16 * B * L.tree_doubles(T, cap)
    assert lib.rnampnn_design_count_long_workspace_bytes(2, T, 1 << 30) == 16 * L.tree_doubles(T, T)      # a cap above T is T


def test_the_bytes_the_header_names_and_zero_for_an_argument_that_is_not_positive(native):
    lib = native.lib()
    assert [lib.rnampnn_design_count_long_workspace_bytes(1, T, cap) for T, cap in ((1025, 1025), (4417, 4417), (4417, 8))] == [172288, 888608,
                                                                                                                                 247728]
    assert L.tree_doubles(1, 1) == 0 and L.tree_doubles(2, 2) == 3
    for fn in (lib.rnampnn_design_count_long_workspace_bytes, lib.rnampnn_design_count_profile_long_workspace_bytes):
        for B, T, cap in ((0, 100, 8), (-1, 100, 8), (2, 0, 8), (2, -5, 8), (2, 100, 0), (2, 100, -1)):
            assert fn(B, T, cap) == 0, (B, T, cap)


def test_header_declares_and_library_exports_the_four_symbols(native):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "rnampnn_hip.h")).read(), flags=re.S)
    for name, kind, n_params in (("rnampnn_design_count_long", "int", 27), ("rnampnn_design_count_profile_long", "int", 25),
                                 ("rnampnn_design_count_long_workspace_bytes", "size_t", 3),
                                 ("rnampnn_design_count_profile_long_workspace_bytes", "size_t", 3)):
        m = re.search(rf"\b{kind}\s+{name}\s*\(([^;]*)\)\s*;", text)
        assert m, f"include/rnampnn_hip.h does not declare {name}"
        assert len([p for p in m.group(1).split(",") if p.strip()]) == len(native.SYMBOLS[name][1]) == n_params, name
        assert hasattr(native.lib(), name)
    import __graft_entry__ as g
    assert "design_long.hip" in g.SOURCES and os.path.exists(os.path.join(g.CSRC, "design_long.hip"))
    assert "profile_dev.h" in g.HEADERS and os.path.exists(os.path.join(g.CSRC, "profile_dev.h"))


# ---------------------------------------------------------------------------------------------------------------- argument errors
WS = 0x10000                                                       # made-up (never dereferenced) addresses: every case returns before a launch


def _need(native, a, profile):
    fn = native.lib().rnampnn_design_count_profile_long_workspace_bytes if profile else native.lib().rnampnn_design_count_long_workspace_bytes
    return int(fn(a["B"], a["T"], max(a["cap"], 1)))


def _draw(native, **kw):
    a = dict(logits=0x1000, n_rows=64, mask=0x2000, cu=None, B=2, T=8, temperature=1.0, S=4, seed=1, seed_dev=None, allowed=None, partner=None,
             wobble=1, bias=None, per_position=0, counted=0xB000, lo=0x7000, hi=0x8000, cap=8, ws=WS, short=0, seqs=0x3000, seq_nll=0x4000,
             infeasible=0x5000, count=0x9000, miss=0xA000)
    a.update(kw)
    vp = lambda v: None if v is None else C.c_void_p(v)
    return native.lib().rnampnn_design_count_long(
        vp(a["logits"]), a["n_rows"], vp(a["mask"]), vp(a["cu"]), a["B"], a["T"], a["temperature"], a["S"], C.c_uint64(a["seed"]), vp(a["seed_dev"]),
        vp(a["allowed"]), vp(a["partner"]), a["wobble"], vp(a["bias"]), a["per_position"], vp(a["counted"]), vp(a["lo"]), vp(a["hi"]), a["cap"],
        vp(a["ws"]), C.c_size_t(max(_need(native, a, False) - a["short"], 0)), vp(a["seqs"]), vp(a["seq_nll"]), vp(a["infeasible"]), vp(a["count"]),
        vp(a["miss"]), None)


def _profile(native, **kw):
    a = dict(logits=0x1000, n_rows=64, mask=0x2000, cu=None, B=2, T=8, temperature=1.0, allowed=None, partner=None, wobble=1, bias=None,
             per_position=0, counted=0xB000, lo=0x7000, hi=0x8000, cap=8, ws=WS, short=0, marg=0x3000, log_z=0x4000, free=0x5000, ent=0x6000,
             infeasible=0x9000, miss=0xA000)
    a.update(kw)
    vp = lambda v: None if v is None else C.c_void_p(v)
    return native.lib().rnampnn_design_count_profile_long(
        vp(a["logits"]), a["n_rows"], vp(a["mask"]), vp(a["cu"]), a["B"], a["T"], a["temperature"], vp(a["allowed"]), vp(a["partner"]), a["wobble"],
        vp(a["bias"]), a["per_position"], vp(a["counted"]), vp(a["lo"]), vp(a["hi"]), a["cap"], vp(a["ws"]),
        C.c_size_t(max(_need(native, a, True) - a["short"], 0)), vp(a["marg"]), vp(a["log_z"]), vp(a["free"]), vp(a["ent"]), vp(a["infeasible"]),
        vp(a["miss"]), None)


SHARED = [
    (dict(logits=None), "null logits"), (dict(B=0), "empty batch"), (dict(T=0), "empty batch"),
    (dict(counted=None), "null counted, count_lo or count_hi"), (dict(lo=None), "null counted, count_lo or count_hi"),
    (dict(hi=None), "null counted, count_lo or count_hi"), (dict(cap=-1), "count_cap = -1"),
    (dict(mask=None, cu=None), "exactly one of mask"), (dict(cu=0x6000), "exactly one of mask"),
    (dict(temperature=0.0), "temperature"), (dict(temperature=float("nan")), "temperature"),
    (dict(logits=0x1004), "16-byte aligned"), (dict(bias=0x6004, per_position=1), "16-byte aligned"),
    (dict(mask=None, cu=0x6000, n_rows=-1), "negative row count"),
    (dict(ws=None), r"the workspace is null \(\d+ bytes\).*needs \d+ \(rnampnn_design_count\w*_long_workspace_bytes\)"),
    (dict(ws=WS + 4), "the workspace must be 8-byte aligned"),
    (dict(short=1), r"the workspace is too small \(\d+ bytes\).*needs \d+"),
    (dict(cap=0, short=1), r"the workspace is too small"),          # count_cap = 0 needs the bytes of count_cap = 1
]


@pytest.mark.parametrize("kw, text", SHARED + [(dict(S=0), "S = 0"), (dict(S=65535), "at most 65534")])
def test_draw_argument_errors_are_value_errors_before_any_launch(native, kw, text):
    rc = _draw(native, **kw)
    assert rc == native.ERR_BAD_ARG
    with pytest.raises(ValueError, match="rnampnn_design_count_long: .*" + text):
        native.check(rc)


@pytest.mark.parametrize("kw, text", SHARED + [(dict(marg=0x3008), "marginals must be 16-byte aligned")])
def test_profile_argument_errors_are_value_errors_before_any_launch(native, kw, text):
    rc = _profile(native, **kw)
    assert rc == native.ERR_BAD_ARG
    with pytest.raises(ValueError, match="rnampnn_design_count_profile_long: .*" + text):
        native.check(rc)


def test_a_call_with_every_output_null_returns_ok_without_a_launch(native):
    assert _draw(native, seqs=None, seq_nll=None, infeasible=None, count=None, miss=None) == 0
    assert _draw(native, T=100000, cap=8, seqs=None, seq_nll=None, infeasible=None, count=None, miss=None) == 0
    assert _profile(native, marg=None, log_z=None, free=None, ent=None, infeasible=None, miss=None) == 0
    assert _draw(native, short=1, seqs=None, seq_nll=None, infeasible=None, count=None, miss=None) == native.ERR_BAD_ARG


def _walk_bytes(T):
    """The walk kernel's LDS formula of include/rnampnn_hip.h, on the host."""
    return 2 * ((4 * ((T + 1) // 2) + 15) & ~15) + ((T + 15) & ~15) + 96


def test_the_limits_are_far_beyond_the_training_set_and_named_in_the_refusal(native):
    assert _walk_bytes(T_MAX_WALK) == 163824 <= 163840 < _walk_bytes(T_MAX_WALK + 1) and _walk_bytes(8192) == 41056 and T_MAX_WALK >= 8192
    for cap in (8, 1 << 30):
        rc = _draw(native, T=T_MAX_WALK + 1, cap=cap)
        assert rc == native.ERR_UNSUPPORTED
        with pytest.raises(NotImplementedError, match=rf"rnampnn_design_count_long: T = {T_MAX_WALK + 1} needs {_walk_bytes(T_MAX_WALK + 1)} bytes of LDS "
                                                      rf".* the limit is 163840 \(T <= {T_MAX_WALK};"):
            native.check(rc)
    rc = _profile(native, T=65537, cap=8)
    assert rc == native.ERR_UNSUPPORTED
    with pytest.raises(NotImplementedError, match=r"rnampnn_design_count_profile_long: T = 65537 lies above 65536"):
        native.check(rc)


def test_the_lds_entries_keep_their_messages_one_past_their_limits(native):
    """What ``tree="lds"``, the default, raises at T = 1018: the size checks precede the launch, so made-up addresses do."""
    vp = lambda v: None if v is None else C.c_void_p(v)
    rc = native.lib().rnampnn_design_gc(vp(0x1000), 64, vp(0x2000), None, 1, 1018, 1.0, 2, C.c_uint64(1), None, None, None, 1, None, 0, vp(0x7000),
                                        vp(0x8000), vp(0x3000), vp(0x4000), vp(0x5000), vp(0x9000), vp(0xA000), None)
    assert rc == native.ERR_UNSUPPORTED
    with pytest.raises(NotImplementedError, match=r"rnampnn_design_gc: T = 1018 needs 163960 bytes of LDS for the count tree, the limit is 163840 \(T <= 1017\)"):
        native.check(rc)
    rc = native.lib().rnampnn_design_count(vp(0x1000), 64, vp(0x2000), None, 1, 1018, 1.0, 2, C.c_uint64(1), None, None, None, 1, None, 0, vp(0xB000),
                                           vp(0x7000), vp(0x8000), 1018, vp(0x3000), vp(0x4000), vp(0x5000), vp(0x9000), vp(0xA000), None)
    with pytest.raises(NotImplementedError, match=r"rnampnn_design_count: T = 1018 at count_cap = 1018 needs 163960 bytes of LDS for the count tree, the "
                                                  r"limit is 163840 \(T <= 1017 at that cap\)"):
        native.check(rc)


# ---------------------------------------------------------------------------------------------------------------- the keyword
def test_tree_chooses_the_entry_and_lds_never_falls_back():
    from rnampnn.model import decode as D
    calls = []

    def refuses_lds(long):
        calls.append(long)
        if not long:
            raise NotImplementedError("rnampnn_design_gc: T = 1018 needs 163960 bytes of LDS")
        return "long"
    with pytest.raises(NotImplementedError, match="T = 1018 needs 163960"):
        D._by_tree("lds", refuses_lds)
    assert calls == [False]
    assert D._by_tree("auto", refuses_lds) == "long" and calls == [False, False, True]
    assert D._by_tree("global", refuses_lds) == "long" and calls[3:] == [True]
    assert D._by_tree("auto", lambda long: ("lds", long)) == ("lds", False)
    with pytest.raises(ValueError, match=r"tree must be one of \['lds', 'global', 'auto'\], got 'hbm'"):
        D._by_tree("hbm", refuses_lds)


def test_tree_with_a_mode_that_has_no_count_tree_is_refused_without_touching_a_device(monkeypatch):
    from rnampnn import _native
    from rnampnn.model import decode as D
    monkeypatch.setattr(_native, "lib", lambda: pytest.fail("the library was loaded"))
    for mode, what in (("states", "states"), ("distinct", "distinct"), ("avoid", "avoid"), ("require", "require"), ("nested", "pairs"),
                       ("plain", "a draw without a count window")):
        for tree in ("global", "auto"):
            with pytest.raises(ValueError, match=f"tree='{tree}' together with {what} is not built: only the count tree"):
                D.check_tree(tree, mode)
        assert D.check_tree("lds", mode) == "lds"
    assert [D.check_tree(tree, mode) for tree in D.TREES for mode in D.TREE_MODES] == ["lds", "lds", "global", "global", "auto", "auto"]
    lg, mask = torch.zeros(1, 8, 4), torch.ones(1, 8)
    with pytest.raises(ValueError, match="tree='global' together with states is not built"):
        D.design_by_mode("states", lg, mask=mask, states=[1], tree="global")
    with pytest.raises(ValueError, match="tree='auto' together with avoid is not built"):
        D.design_profile_from_logits(lg, mask=mask, avoid=["GGGG"], tree="auto")
    with pytest.raises(ValueError, match="tree must be one of"):
        D.design_gc_from_logits(lg, mask=mask, tree="hbm")
    with pytest.raises(ValueError, match="tree must be one of"):
        D.design_count_from_logits(lg, mask=mask, counted=torch.zeros(1, 8, dtype=torch.uint8), tree="hbm")
    for tree in D.TREES:                                            # the count modes get as far as the device check
        with pytest.raises(RuntimeError, match="runs on an MI355X"):
            D.design_gc_from_logits(lg, mask=mask, tree=tree)
        with pytest.raises(RuntimeError, match="runs on an MI355X"):
            D.design_mutations_from_logits(lg, (torch.zeros(1, 8, dtype=torch.int64), (0, 2)), mask=mask, tree=tree)
        with pytest.raises(RuntimeError, match="runs on an MI355X"):
            D.design_profile_from_logits(lg, mask=mask, tree=tree)


def test_the_models_refuse_before_their_forward_pass(monkeypatch):
    from rdesign.model.rdesign import RNAModel
    from rnampnn.model.rnampnn import RNAMPNN
    for cls in (RNAMPNN, RNAModel):
        def forward_ran(*a, **k):
            pytest.fail("the forward pass ran")
        for name in ("_run", "_packed_logits"):
            if hasattr(cls, name):
                monkeypatch.setattr(cls, name, forward_ran)
        model = cls.__new__(cls)
        x, mask = torch.zeros(2, 8, 7, 3), torch.ones(2, 8)
        for kw, what in ((dict(states=[2]), "states"), (dict(distinct="sample"), "distinct"), (dict(avoid=["GGGG"]), "avoid"),
                         (dict(require=["GGAGG"]), "require"), (dict(pairs="nested", avoid=["GGGG"]), "pairs"),
                         ({}, "a draw without a count window")):
            with pytest.raises(ValueError, match=f"tree='global' together with {what} is not built"):
                cls.design(model, x, mask, tree="global", **kw)
        with pytest.raises(ValueError, match="tree must be one of"):
            cls.design(model, x, mask, gc_content=(0.4, 0.6), tree="hbm")
        with pytest.raises(ValueError, match="tree='auto' together with avoid is not built"):
            cls.design_profile(model, x, mask, avoid=["GGGG"], tree="auto")


def test_the_cli_refuses_before_a_checkpoint_is_opened():
    import predict as P
    base = ["--ckpt", "/nonexistent.pt", "--data", "none", "--samples", "2"]
    assert P.parse(base).tree is None and P.tree_option(P.parse(base)) == {}
    assert P.tree_option(P.parse(base + ["--gc-content", "0.45:0.60", "--tree", "auto"])) == {"tree": "auto"}
    assert P.tree_option(P.parse(base + ["--max-mutations", "8", "--tree", "global"])) == {"tree": "global"}
    assert P.tree_option(P.parse(base + ["--states", "s.csv", "--tree", "lds"])) == {"tree": "lds"}
    for flags in (["--states", "s.csv"], ["--avoid", "GGGG"], ["--distinct", "sample"], ["--require", "GGAGG"], ["--max-run", "3"],
                  ["--pairs", "nested", "--avoid", "GGGG"]):
        for tree in ("global", "auto"):
            with pytest.raises(ValueError, match=f"--tree {tree} together with {flags[0]} is not built"):
                P.run(P.parse(base + flags + ["--tree", tree]))
    with pytest.raises(ValueError, match="--tree global needs --gc-content or --max-mutations"):
        P.run(P.parse(base + ["--tree", "global"]))
    with pytest.raises(SystemExit):
        P.parse(base + ["--tree", "hbm"])


# ---------------------------------------------------------------------------------------------------------------- the device tests' cases
@pytest.mark.parametrize("name", ["gc1018", "gc1025", "gc2049", "mut2868", "mixed"])
def test_no_reference_draw_of_the_long_cases_passes_near_a_boundary(name):
    """The device tests leave no draw out, so every selection of the restatement's draws must lie further than NEAR from a cumulative
    boundary; each case also has its hairpin across the root's boundary and its IUPAC stripe."""
    c = L.case(name)
    seqs, margin, bad, miss, plans = L.draw_ref(name)
    print(f"{name}: the smallest margin {margin.min():.3e}")
    assert margin.min() > L.NEAR
    for b, n in enumerate(c["lengths"]):
        if n >= 64:
            mid = 1 << ((n - 1).bit_length() - 1)
            assert any(i < mid <= j for i, j in L.hairpin(n)) and (c["allowed"][b, 8:48] != 15).sum() >= 35
            assert all(c["partner"][b, i] == j and c["partner"][b, j] == i for i, j in L.hairpin(n))
    assert bad.tolist() == [0] * c["B"]
    assert (miss.tolist() == [0, 108] and plans[1].at_min) if name == "mut2868" else miss.tolist() == [0] * c["B"]
