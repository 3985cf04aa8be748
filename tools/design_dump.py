#!/usr/bin/env python3
"""Every output of the design wrappers on the batches of the GPU tests, as .npy files: the byte comparison of two builds of the library
(docs/experiments.md, "the design family folded").  Plain dumping - no timing, no profiler, no retry.
usage: python tools/design_dump.py <outdir>            one child process per family (design tied gc count distinct avoid profile dfa nested
                                                       chain dfa_profile), each under its own
                                                       `timeout`, stopping at the first that fails; then the number of dumps, their size
                                                       and one sha256 over all of them
       python tools/design_dump.py <outdir> <family>   that family, in this process
RNAMPNN_PROBE_ROOT: another checkout (with its library built) to take the package from, as in tools/design_probe.py - the batches always
come from THIS checkout's tests/, and only API that the parent of this tool's commit has is used.  Compare two runs with
`diff -r <outdir a> <outdir b>` or by the printed sha256.
Per family the `host_case()` / `case_arrays()` batch of its GPU test file, every constraint variant that file defines, temperatures 1.0,
0.3 and 1e-3, the padded and the packed layout, the file's seed (above 2^32); tied: STATES with its weights and one state per group;
gc: the case's windows as fractions, 40..60 % and the free window; count: caps 8 and T; distinct: S = 8 and 64, "sample" and "best";
avoid: every automaton of CASE_AUTOMATA under the case's sets and bias, and free; profile: the six outputs of `design_profile_from_logits`
in the modes plain / gc_content / mutations on the count batch (the latter two with the tree in LDS and in global memory) and avoid on
the avoid batch; dfa, nested, chain: every automaton of the file's CASE_AUTOMATA under the case's constraints (nested: the structure
included; chain: a G+C window and the two mutation budgets of CASE_SIDES); dfa_profile: the six outputs under `table="global"` for every
automaton of the dfa batch and for the avoid batch's automata.
With every set of draws the `seq_nll` that `score_logits` gives for it."""
import hashlib
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.environ.get("RNAMPNN_PROBE_ROOT") or os.path.join(HERE, "..")
FAMILIES = ("design", "tied", "gc", "count", "distinct", "avoid", "profile", "dfa", "nested", "chain", "dfa_profile")
TEMPERATURES = (1.0, 0.3, 1e-3)


def dump_family(outdir: str, family: str) -> None:
    sys.path.insert(0, os.path.join(ROOT, "rna-mpnn_amd"))
    import numpy as np
    import torch
    from rnampnn import _native
    from rnampnn.model import decode as D
    from rnampnn.utils.constraints import DesignConstraints
    assert os.path.realpath(_native.__file__).startswith(os.path.realpath(ROOT)), (_native.__file__, ROOT)
    _native.lib()
    sys.path.insert(0, os.path.join(HERE, "..", "tests"))               # (the package is imported: these only add the batches)
    os.makedirs(outdir, exist_ok=True)

    def save(tag, names, outs, logits_kw=None):
        outs, names = list(outs), tuple(names)
        if logits_kw is not None:                                       # draws: their score as rnampnn_score gives it
            outs.append(D.score_logits(seqs=outs[0], want=("seq_nll",), **logits_kw)["seq_nll"])
            names += ("score_seq_nll",)
        for name, t in zip(names, outs):
            np.save(os.path.join(outdir, f"{family}.{tag}.{name}.npy"), t.cpu().numpy())

    def automata(A):
        from rnampnn.utils.motifs import MotifAutomaton
        return {name: MotifAutomaton.from_motifs(motifs, max_run=max_run) for name, (motifs, max_run) in A.CASE_AUTOMATA.items()}

    def layouts(h, T):
        dev = {k: torch.from_numpy(h[k]).cuda() for k in ("logits", "mask", "packed", "cu")}
        return (("padded", dict(logits=dev["logits"], mask=dev["mask"])), ("packed", dict(logits=dev["packed"], cu_seqlens=dev["cu"], max_len=T)))

    def constraints(h, bias, wobble):
        return DesignConstraints(torch.from_numpy(h["allowed"]), torch.from_numpy(h["partner"]), None if bias is None else torch.from_numpy(bias),
                                 wobble).to_device("cuda")

    triple = ("seqs", "seq_nll", "infeasible")
    if family in ("design", "tied"):
        mod = __import__("test_design_gpu" if family == "design" else "test_design_tied_gpu")
        h = mod.host_case()
        variants = {name: constraints(h, None if v["bias"] is None else h[v["bias"]], v["wobble"]) for name, v in mod.VARIANTS.items()}
        variants["free"] = None
        one = [1] * h["B"]
        states = {"rows": dict(), "one": dict(states=one)} if family == "design" else {
            "states": dict(states=mod.STATES, state_weights=torch.from_numpy(h["weight"]).cuda()), "one": dict(states=one)}
        for vname, cons in variants.items():
            for temperature in TEMPERATURES:
                for lname, kw in layouts(h, mod.T):
                    for sname, skw in states.items():
                        out = D.design_from_logits(n_samples=mod.S, temperature=temperature, seed=mod.SEED, constraints=cons, **kw, **skw)
                        save(f"{vname}.t{temperature:g}.{lname}.{sname}", triple, out, kw)
    elif family == "gc":
        import _design_gc_ref as G
        h = G.case_arrays()
        n = np.maximum(np.array(G.CASE_LENGTHS, dtype=np.float64), 1.0)
        case_window = torch.from_numpy(np.stack([h["lo"] / n, h["hi"] / n], axis=1)).cuda()     # (not read back: the kernel clamps it)
        windows = {"case": case_window, "40-60": (0.4, 0.6), "all": (0.0, 1.0)}
        variants = {"cons": constraints(h, None, True), "bias": constraints(h, G.CASE_BIAS, True), "free": None}
        for vname, cons in variants.items():
            for temperature in TEMPERATURES:
                for lname, kw in layouts(h, G.CASE_T):
                    for wname, window in windows.items():
                        out = D.design_gc_from_logits(n_samples=G.CASE_S, temperature=temperature, seed=G.CASE_SEED, constraints=cons,
                                                      gc_content=window, **kw)
                        save(f"{vname}.t{temperature:g}.{lname}.{wname}", triple + ("gc_count", "gc_miss"), out, kw)
    elif family == "count":
        import _design_count_ref as R
        h = R.case_arrays()
        counted = torch.from_numpy(h["counted"]).cuda()
        window = torch.from_numpy(np.stack([h["lo"], h["hi"]], axis=1)).cuda()
        variants = {"cons": constraints(h, None, R.CASE_WOBBLE), "wobble": constraints(h, None, True), "free": None}
        for vname, cons in variants.items():
            for temperature in TEMPERATURES:
                for lname, kw in layouts(h, R.CASE_T):
                    for cap in R.CASE_CAPS:
                        out = D.design_count_from_logits(n_samples=R.CASE_S, temperature=temperature, seed=R.CASE_SEED, constraints=cons,
                                                         counted=counted, window=window, cap=cap, **kw)
                        save(f"{vname}.t{temperature:g}.{lname}.cap{cap}", triple + ("count", "count_miss"), out, kw)
    elif family == "distinct":
        import _design_distinct_ref as X
        h = X.case_arrays()
        variants = {"cons": constraints(h, None, True), "nowobble": constraints(h, None, False), "free": None}
        for vname, cons in variants.items():
            for temperature in TEMPERATURES:
                for lname, kw in layouts(h, X.CASE_T):
                    for S in (8, 64):
                        for mode in ("sample", "best"):
                            out = D.design_distinct_from_logits(n_samples=S, temperature=temperature, seed=X.CASE_SEED, constraints=cons,
                                                                mode=mode, **kw)
                            save(f"{vname}.t{temperature:g}.{lname}.S{S}.{mode}", triple + ("logp", "n_distinct"), out, kw)
    elif family == "avoid":
        import _design_avoid_ref as A
        h = A.case_arrays()
        variants = {"cons": DesignConstraints(torch.from_numpy(h["allowed"]), None, torch.from_numpy(h["bias"]), True).to_device("cuda"), "free": None}
        for vname, cons in variants.items():
            for aname, auto in automata(A).items():
                for temperature in TEMPERATURES:
                    for lname, kw in layouts(h, A.CASE_T):
                        out = D.design_avoid_from_logits(n_samples=A.CASE_S, temperature=temperature, seed=A.CASE_SEED, constraints=cons,
                                                         avoid=auto, **kw)
                        save(f"{vname}.{aname}.t{temperature:g}.{lname}", triple + ("hits", "avoid_miss"), out, kw)
    elif family == "profile":
        import _design_avoid_ref as A
        import _design_count_ref as R
        six = ("marginals", "log_z", "log_z_free", "entropy", "infeasible", "miss")
        h, ha = R.case_arrays(), A.case_arrays()
        reference = torch.from_numpy(h["reference"]).cuda()
        modes = {"plain": dict(), "gc_content": dict(gc_content=(0.4, 0.6)), "mutations": dict(mutations=(reference, 0, 8)),
                 "gc_content_long": dict(gc_content=(0.4, 0.6), tree="global"), "mutations_long": dict(mutations=(reference, 0, 8), tree="global")}
        variants = {"cons": constraints(h, None, R.CASE_WOBBLE), "wobble": constraints(h, None, True), "free": None}
        for vname, cons in variants.items():
            for mname, mkw in modes.items():
                for temperature in TEMPERATURES:
                    for lname, kw in layouts(h, R.CASE_T):
                        out = D.design_profile_from_logits(temperature=temperature, constraints=cons, **mkw, **kw)
                        save(f"{mname}.{vname}.t{temperature:g}.{lname}", six, out[:6])
        variants = {"cons": DesignConstraints(torch.from_numpy(ha["allowed"]), None, torch.from_numpy(ha["bias"]), True).to_device("cuda"), "free": None}
        for vname, cons in variants.items():
            for aname, auto in automata(A).items():
                for temperature in TEMPERATURES:
                    for lname, kw in layouts(ha, A.CASE_T):
                        out = D.design_profile_from_logits(temperature=temperature, constraints=cons, avoid=auto, **kw)
                        save(f"avoid.{vname}.{aname}.t{temperature:g}.{lname}", six, out[:6])
    elif family in ("dfa", "nested", "chain"):
        from rnampnn.utils.motifs import DesignAutomaton, as_nested_automaton
        R = __import__({"dfa": "_design_dfa_ref", "nested": "_design_nested_ref", "chain": "_design_dfa_count_ref"}[family])
        h = R.case_arrays()
        partner = torch.from_numpy(h["partner"]) if family == "nested" else None
        cons = DesignConstraints(torch.from_numpy(h["allowed"]), partner, torch.from_numpy(h["bias"]), True).to_device("cuda")
        further = {"dfa": ("hits", "accepted", "dfa_miss"), "nested": ("hits", "accepted", "dfa_miss", "nest_miss"),
                   "chain": ("hits", "accepted", "count", "dfa_miss", "count_miss", "log_z")}[family]
        sides = {"draw": dict()}
        if family == "chain":
            reference = torch.from_numpy(h["reference"]).cuda()
            sides = {"gc": dict(gc_content=(0.4, 0.6)), "mut4": dict(mutations=(reference, (0, 4))), "mut2_6": dict(mutations=(reference, (2, 6)))}
        call = {"dfa": D.design_dfa_from_logits, "nested": D.design_nested_from_logits, "chain": D.design_dfa_count_from_logits}[family]
        for aname, (require, avoid, max_run) in R.CASE_AUTOMATA.items():
            auto = DesignAutomaton.from_motifs(require, avoid, max_run) if family == "dfa" else as_nested_automaton(require or None, avoid or None, max_run)
            for temperature in TEMPERATURES:
                for lname, kw in layouts(h, R.CASE_T):
                    for sname, skw in sides.items():
                        out = call(n_samples=R.CASE_S, temperature=temperature, seed=R.CASE_SEED, constraints=cons, require=auto, **skw, **kw)
                        save(f"{aname}.t{temperature:g}.{lname}.{sname}", triple + further, out, kw)
    elif family == "dfa_profile":
        import _design_avoid_ref as A
        import _design_dfa_ref as R
        from rnampnn.utils.motifs import DesignAutomaton
        six = ("marginals", "log_z", "log_z_free", "entropy", "infeasible", "miss")
        for bname, B, autos in (("require", R, {n: dict(require=DesignAutomaton.from_motifs(*spec)) for n, spec in R.CASE_AUTOMATA.items()}),
                                ("avoid", A, {n: dict(avoid=a) for n, a in automata(A).items()})):
            h = B.case_arrays()
            cons = DesignConstraints(torch.from_numpy(h["allowed"]), None, torch.from_numpy(h["bias"]), True).to_device("cuda")
            for aname, akw in autos.items():
                for temperature in TEMPERATURES:
                    for lname, kw in layouts(h, B.CASE_T):
                        out = D.design_profile_from_logits(temperature=temperature, constraints=cons, table="global", **akw, **kw)
                        save(f"{bname}.{aname}.t{temperature:g}.{lname}", six, out[:6])
    else:
        raise SystemExit(f"unknown family {family!r}: choose from {FAMILIES}")
    torch.cuda.synchronize()
    print(f"{family}: dumped from {os.path.realpath(_native.LIB_PATH)}")


def main() -> int:
    if len(sys.argv) < 2:
        raise SystemExit(__doc__)
    outdir = os.path.abspath(sys.argv[1])
    if len(sys.argv) > 2:
        dump_family(outdir, sys.argv[2])
        return 0
    for family in FAMILIES:
        rc = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.abspath(__file__), outdir, family]).returncode
        if rc != 0:
            print(f"{family}: exit status {rc}; nothing further is started")
            return rc
    files = sorted(f for f in os.listdir(outdir) if f.endswith(".npy"))
    digest, size = hashlib.sha256(), 0
    for f in files:
        data = open(os.path.join(outdir, f), "rb").read()
        digest.update(f.encode() + b"\0" + data)
        size += len(data)
    print(f"{len(files)} dumps, {size} bytes, sha256 {digest.hexdigest()}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
