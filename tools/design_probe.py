#!/usr/bin/env python3
"""The measurement behind DESIGN.md section 9 "Constrained design", "Multi-state design", "Design under a G+C window", "Distinct designs",
"Mutation budget", "Forbidden motifs", "Required motifs", "Motifs under a nested structure", "Design profiles" and "Count tree in global memory" (profiles/design_long_kernel_stats.txt, profiles/design_nested_kernel_stats.txt, profiles/design_dfa_kernel_stats.txt, profiles/design_profile_kernel_stats.txt, profiles/design_kernel_stats.txt, profiles/design_tied_kernel_stats.txt, profiles/design_gc_kernel_stats.txt,
profiles/design_distinct_kernel_stats.txt, profiles/design_count_kernel_stats.txt, profiles/design_avoid_kernel_stats.txt): the C2 batch (256 RNAs x 100..140 nt), S = 8 sequences per RNA.
usage: python tools/design_probe.py sample_score [calls=50]   rnampnn_sample + rnampnn_score (seq_nll): the unconstrained pair of launches
       python tools/design_probe.py design [calls=50]         rnampnn_design: free, then with a hairpin's pairs + a fixed GNRA loop per RNA
       python tools/design_probe.py tied [calls=50]           rnampnn_design (free, hairpin) and then rnampnn_design_tied: one state per group
                                                              free, one state per group with the hairpins, 64 groups x 4 states with one 3-node chain
       python tools/design_probe.py gc [calls=50]             rnampnn_design (free, hairpin) and then rnampnn_design_gc with the window 40..60 %:
                                                              free, then with the hairpins
       python tools/design_probe.py count                     rnampnn_design (free, hairpin) and then, in 5 alternating rounds of 10 calls each,
                                                              rnampnn_design_gc 40..60 % and rnampnn_design_count: (a) C|G counted, cap T, the
                                                              same windows (the work of rnampnn_design_gc), each free and with the hairpins;
                                                              (b) at most 8 mutations from a random reference, cap 8, free; (c) the same budget
                                                              with the hairpins and a reference that is compatible with them
       python tools/design_probe.py distinct [calls=50]       rnampnn_design (free, hairpin) and then rnampnn_design_distinct at S = 8 and S = 64,
                                                              "sample" then "best", each free and then with the hairpins (8 legs)
       python tools/design_probe.py avoid                     rnampnn_design (free, hairpin) and then, in 5 alternating rounds of 10 calls each,
                                                              rnampnn_design_count (b) (S = 8, cap 8: the yardstick) and rnampnn_design_avoid:
                                                              S = 8 with max_run = 3 (13 live states), S = 8 with a 64-state set, S = 64 with
                                                              max_run = 3; all without constraints
       python tools/design_probe.py profile                   rnampnn_design (free, hairpin) and then, in 5 alternating rounds of 10 calls each,
                                                              the two draw entries as yardsticks of the same run - rnampnn_design_count (b)
                                                              and rnampnn_design_avoid max_run = 3, S = 8 - and the profile entries:
                                                              rnampnn_design_count_profile with the G+C window 40..60 % (cap T), with 0..8
                                                              mutations (cap 8) and plain under the hairpins (cap 0);
                                                              rnampnn_design_avoid_profile with max_run = 3 and with the 64-state set
       python tools/design_probe.py dfa                       rnampnn_design (free, hairpin) and then, in 5 alternating rounds of 10 calls each,
                                                              rnampnn_design_avoid max_run = 3, S = 8 (the yardstick) and rnampnn_design_dfa:
                                                              the same automaton with every live state accepting (the same work, the table
                                                              in global memory), require GGAGG + max_run = 3, and require GGAGG and CUUCG +
                                                              max_run = 3 (89 states); then the yield of filtering free draws for GGAGG
       python tools/design_probe.py nested                    rnampnn_design (free, hairpin) and then, in 5 alternating rounds of 10 calls each,
                                                              rnampnn_design_dfa max_run = 3 with every live state accepting, S = 8 (the
                                                              yardstick) and rnampnn_design_nested: the same automaton without pairs (the
                                                              same work), the same automaton under a hairpin-rich nested structure on every
                                                              RNA (13 live states), and require GNRA + max_run = 3 under that structure (53)
       python tools/design_probe.py chain                     rnampnn_design (free, hairpin) and then, in 5 alternating rounds of 10 calls each,
                                                              the yardsticks of the same run - rnampnn_design_dfa max_run = 3 with every live
                                                              state accepting, rnampnn_design_count under the G+C window 45..60 % (cap T) and
                                                              under 0..8 mutations (cap 8), S = 8 - and rnampnn_design_dfa_count on that
                                                              automaton: nothing counted (the work of rnampnn_design_dfa), under that G+C
                                                              window, and under that budget (profiles/design_dfa_count_kernel_stats.txt)
       python tools/design_probe.py dfa_profile               rnampnn_design (free, hairpin) and then, in 5 alternating rounds of 10 calls each,
                                                              the yardsticks of the same run - rnampnn_design_dfa, S = 8, at max_run = 3 with
                                                              every live state accepting (13 live states), require GGAGG and CUUCG +
                                                              max_run = 3 (73) and two long required words (256), and
                                                              rnampnn_design_avoid_profile max_run = 3 - and rnampnn_design_dfa_profile at the
                                                              three automata; then one RNA of 4,498 nt, the largest it accepts
                                                              (profiles/design_dfa_profile_kernel_stats.txt)
       python tools/design_probe.py long                      the count tree in global memory (tree="global": rnampnn_design_count_long,
                                                              rnampnn_design_count_profile_long), nothing else: (a) the C2 batch in 5
                                                              alternating rounds of 10 calls - rnampnn_design_gc 40..60 %, rnampnn_design_count
                                                              (b) and the G+C profile, each through the LDS entry and through the long entry
                                                              on the same inputs; (b) one RNA of 4,417 nt, S = 8: a G+C window of 45..60 %, a
                                                              budget of 8 mutations and the G+C profile; (c) a padded batch of the 32 longest
                                                              lengths of tests/data/c3_train_lengths.npy under the G+C window.  Every chunk of
                                                              calls is logged in order ("long-calls|name|calls") for tools/kstats_design.sh
HIP events around each loop of back-to-back calls of the Python wrappers.  Run either under `rocprofv3 --kernel-trace --stats -- python ...`
(a run of its own) for the kernels' own times.  RNAMPNN_PROBE_ROOT: another checkout (with its library built) to take the package from -
the `sample_score` leg uses nothing newer than rnampnn_score, so it runs on the parent commit as well."""
import os
import sys

REPO = os.environ.get("RNAMPNN_PROBE_ROOT") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(REPO, "rna-mpnn_amd"))
import torch
from rnampnn.model import rnampnn as M
from rnampnn.utils import synth

what = sys.argv[1] if len(sys.argv) > 1 else "design"
n_calls = int(sys.argv[2]) if len(sys.argv) > 2 else 50
S = 8
lens = [int(n) for n in synth.synth_lengths(256, 100, 140, seed=0)]
_, mask, _ = synth.synth_batch(lens)
B, T = mask.shape
m = torch.from_numpy(mask).cuda()
logits = (3.0 * torch.randn(B, T, 4, generator=torch.Generator().manual_seed(0))).cuda() * m[..., None]


def timed(name, fn):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n_calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    print(f"B {B} T {T} nt {int(mask.sum())} S {S} {name}: {e0.elapsed_time(e1) * 1e3 / n_calls:.2f} us per call (events, back to back, "
          f"output allocation included)")


def long_leg():
    import numpy as np
    from rnampnn.model import decode as D
    rounds, per_round, warm = 5, 10, 3

    def chunk(name, fn, calls):
        """``calls`` back-to-back calls between two events -> us per call; the chunk is logged in execution order."""
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        torch.cuda.synchronize()
        print(f"long-calls|{name}|{calls}")
        return e0.elapsed_time(e1) * 1e3 / calls

    def once(name, fn):
        """One call outside the timing, logged like a chunk so that the order of the log stays the order of the launches."""
        out = fn()
        torch.cuda.synchronize()
        print(f"long-calls|{name} (check)|1")
        return out

    def report(tag, shape, variants, times):
        for (name, _), t in zip(variants, times):
            print(f"{tag} {shape} S {S} {name}: {sum(t) / len(t):.2f} us per call, rounds {min(t):.2f} .. {max(t):.2f} ({len(t)} round(s), events, "
                  f"output and workspace allocation included)")

    kw = dict(n_samples=S, temperature=0.1, seed=1)
    ref = torch.randint(0, 4, (B, T), generator=torch.Generator().manual_seed(1)).cuda()
    sets = D.mutation_sets(ref)
    a = [(f"{entry}, {tree}", fn) for entry, make in (
        ("gc 40..60 %", lambda tree: lambda: D.design_gc_from_logits(logits, mask=m, gc_content=(0.4, 0.6), tree=tree, **kw)),
        ("count (b) 0..8 mutations cap 8", lambda tree: lambda: D.design_count_from_logits(logits, mask=m, counted=sets, window=(0, 8), tree=tree, **kw)),
        ("profile G+C 40..60 %", lambda tree: lambda: D.design_profile_from_logits(logits, mask=m, temperature=0.1, gc_content=(0.4, 0.6), tree=tree)))
         for tree, fn in (("lds", make("lds")), ("global", make("global")))]
    for name, fn in a:
        chunk(name + " (warm)", fn, warm)
    times = [[] for _ in a]
    for _ in range(rounds):
        for v, (name, fn) in enumerate(a):
            times[v].append(chunk(name, fn, per_round))
    report("(a)", f"B {B} T {T} nt {int(mask.sum())}", a, times)
    for (n0, f0), (n1, f1) in zip(a[0::2], a[1::2]):
        x, y = once(n0, f0), once(n1, f1)
        print(f"{n1} against {n0}: " + ", ".join(f"{k} equal {bool((p == q).all())}" for k, p, q in zip(
            ("seqs / marginals", "seq_nll / log_z", "infeasible / log_z_free", "count / entropy", "miss / infeasible", "- / miss"), x, y)))
    # (b) one ribosomal-size RNA
    n1 = 4417
    lg1 = 3.0 * torch.randn(1, n1, 4, generator=torch.Generator().manual_seed(2)).cuda()
    m1 = torch.ones(1, n1, device="cuda")
    ref1 = torch.randint(0, 4, (1, n1), generator=torch.Generator().manual_seed(3)).cuda()
    b = [("gc 45..60 %, 4417 nt, global", lambda: D.design_gc_from_logits(lg1, mask=m1, gc_content=(0.45, 0.60), tree="global", **kw)),
         ("mutations 0..8 cap 8, 4417 nt, global", lambda: D.design_mutations_from_logits(lg1, (ref1, (0, 8)), mask=m1, tree="global", **kw)),
         ("profile G+C 45..60 %, 4417 nt, global", lambda: D.design_profile_from_logits(lg1, mask=m1, temperature=0.1, gc_content=(0.45, 0.60), tree="global"))]
    for name, fn in b:
        chunk(name + " (warm)", fn, 2)
    report("(b)", f"B 1 T {n1}", b, [[chunk(name, fn, 10)] for name, fn in b])
    out, mut = once(b[0][0], b[0][1]), once(b[1][0], b[1][1])
    print(f"(b) G+C of the 4,417-nt draws {out[3].min().item() / n1:.4f} .. {out[3].max().item() / n1:.4f}, gc_miss {out[4].tolist()}; "
          f"mutations {mut[3].tolist()}; workspace {int(D._native.lib().rnampnn_design_count_long_workspace_bytes(1, n1, n1))} / "
          f"{int(D._native.lib().rnampnn_design_count_long_workspace_bytes(1, n1, 8))} bytes uncapped / cap 8")
    # (c) the 32 longest RNAs of the training set, one padded batch
    lens32 = sorted(int(v) for v in np.load(os.path.join(REPO, "tests", "data", "c3_train_lengths.npy")))[-32:]
    m32 = torch.zeros(32, max(lens32))
    for r, n in enumerate(lens32):
        m32[r, :n] = 1
    m32 = m32.cuda()
    lg32 = 3.0 * torch.randn(32, max(lens32), 4, generator=torch.Generator().manual_seed(4)).cuda() * m32[..., None]
    c = [("gc 45..60 %, 32 longest, global", lambda: D.design_gc_from_logits(lg32, mask=m32, gc_content=(0.45, 0.60), tree="global", **kw))]
    chunk(c[0][0] + " (warm)", c[0][1], 1)
    report("(c)", f"B 32 T {max(lens32)} nt {sum(lens32)} (lengths {lens32[0]} .. {lens32[-1]})", c, [[chunk(c[0][0], c[0][1], 5)]])
    out = once(c[0][0], c[0][1])
    frac = out[3].double() / m32.sum(dim=1).double()
    print(f"(c) G+C of the draws {float(frac.min()):.4f} .. {float(frac.max()):.4f}, gc_miss total {int(out[4].sum())}, workspace "
          f"{int(D._native.lib().rnampnn_design_count_long_workspace_bytes(32, max(lens32), max(lens32)))} bytes")


if what == "long":
    long_leg()
elif what == "sample_score":
    def two_launches():
        seqs = M.sample_from_logits(logits, m, 0.1, S, seed=1)
        return seqs, M.score_logits(logits, mask=m, seqs=seqs, want=("seq_nll",))["seq_nll"]
    timed("rnampnn_sample + rnampnn_score(seq_nll)", two_launches)
else:
    from rnampnn.utils.constraints import DesignConstraints
    import numpy as np
    specs = []
    for n in lens:                                                  # a hairpin: a stem of (n - 4) // 2 pairs closed by a GNRA tetraloop
        stem = (n - 4) // 2
        specs.append(("." * stem + "GNRA" + "." * (n - stem - 4), "(" * stem + "...." + ")" * stem + "." * (n - 2 * stem - 4)))
    cons = DesignConstraints.from_specs(specs, lens, T, bias=[0.0, 0.0, 0.0, -0.5]).to_device("cuda")
    timed("rnampnn_design, no constraints", lambda: M.design_from_logits(logits, mask=m, n_samples=S, temperature=0.1, seed=1))
    timed("rnampnn_design, hairpin pairs + GNRA + bias", lambda: M.design_from_logits(logits, mask=m, n_samples=S, temperature=0.1, seed=1,
                                                                                      constraints=cons))
    seqs, nll, bad = M.design_from_logits(logits, mask=m, n_samples=S, temperature=0.1, seed=1, constraints=cons)
    print(f"infeasible positions {int(bad.sum())}, mean NLL per nt {float(nll.sum()) / (S * int(mask.sum())):.4f}")
    if what == "gc":
        gc = dict(n_samples=S, temperature=0.1, seed=1, gc_content=(0.4, 0.6))
        timed("rnampnn_design_gc 40..60 %, no constraints", lambda: M.design_gc_from_logits(logits, mask=m, **gc))
        timed("rnampnn_design_gc 40..60 %, hairpin pairs + GNRA + bias", lambda: M.design_gc_from_logits(logits, mask=m, constraints=cons, **gc))
        g_seqs, g_nll, g_bad, g_count, g_miss = M.design_gc_from_logits(logits, mask=m, constraints=cons, **gc)
        frac = g_count.double() / m.sum(dim=1).double()
        print(f"G+C fraction of the draws {float(frac.min()):.3f} .. {float(frac.max()):.3f} (unconstrained hairpin draws: "
              f"{float(((seqs >= 2).sum(-1).double() / m.sum(dim=1).double()).min()):.3f} .. "
              f"{float(((seqs >= 2).sum(-1).double() / m.sum(dim=1).double()).max()):.3f}), gc_miss total {int(g_miss.sum())}, "
              f"infeasible equal {bool((g_bad == bad).all())}, mean NLL per nt {float(g_nll.sum()) / (S * int(mask.sum())):.4f}")
    if what == "count":
        # Six variants in alternating rounds of one process, so that k_design_count is compared with k_design_gc of the SAME run and the
        # round-to-round spread of either is visible: k_design_gc 40..60 % free / hairpins; (a) rnampnn_design_count with C|G counted
        # everywhere, cap = T and the same windows - the work of k_design_gc - free / hairpins; (b) a random reference, at most 8
        # mutations, cap 8, free; (c) the same budget with the hairpins, the reference made compatible with them (complementary over
        # the stem, GAAA in the loop: the structure alone forces no mutation).
        from rnampnn.model import decode as D
        from rnampnn.model.decode import gc_counts, gc_fractions
        rounds, per_round, warm = 5, 10, 3
        kw = dict(n_samples=S, temperature=0.1, seed=1)
        lo, hi = gc_counts(gc_fractions((0.4, 0.6), B).cuda(), m.sum(dim=1))
        window = torch.stack([lo, hi], dim=1)
        cg = torch.full((B, T), 12, dtype=torch.uint8, device="cuda")
        ref = torch.randint(0, 4, (B, T), generator=torch.Generator().manual_seed(1))
        ref_hp = ref.clone()
        for b, n in enumerate(lens):
            stem = (n - 4) // 2
            for i in range(stem):
                ref_hp[b, n - (n - 2 * stem - 4) - 1 - i] = (1, 0, 3, 2)[int(ref_hp[b, i])]
            ref_hp[b, stem:stem + 4] = torch.tensor([3, 0, 0, 0])
        sets, sets_hp = D.mutation_sets(ref.cuda()), D.mutation_sets(ref_hp.cuda())
        variants = [
            ("rnampnn_design_gc 40..60 %, no constraints", lambda: M.design_gc_from_logits(logits, mask=m, gc_content=(0.4, 0.6), **kw)),
            ("rnampnn_design_count (a) C|G counted, cap T, 40..60 %, no constraints",
             lambda: D.design_count_from_logits(logits, mask=m, counted=cg, window=window, cap=T, **kw)),
            ("rnampnn_design_gc 40..60 %, hairpin pairs + GNRA + bias",
             lambda: M.design_gc_from_logits(logits, mask=m, constraints=cons, gc_content=(0.4, 0.6), **kw)),
            ("rnampnn_design_count (a) C|G counted, cap T, 40..60 %, hairpin pairs + GNRA + bias",
             lambda: D.design_count_from_logits(logits, mask=m, constraints=cons, counted=cg, window=window, cap=T, **kw)),
            ("rnampnn_design_count (b) random reference, 0..8 mutations, cap 8, no constraints",
             lambda: D.design_count_from_logits(logits, mask=m, counted=sets, window=(0, 8), **kw)),
            ("rnampnn_design_count (c) compatible reference, 0..8 mutations, cap 8, hairpin pairs + GNRA + bias",
             lambda: D.design_count_from_logits(logits, mask=m, constraints=cons, counted=sets_hp, window=(0, 8), **kw))]
        for _, fn in variants:
            for _ in range(warm):
                fn()
        torch.cuda.synchronize()
        times = [[] for _ in variants]
        for _ in range(rounds):
            for v, (_, fn) in enumerate(variants):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(per_round):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                times[v].append(e0.elapsed_time(e1) * 1e3 / per_round)
        for (name, _), t in zip(variants, times):
            print(f"B {B} T {T} nt {int(mask.sum())} S {S} {name}: {sum(t) / len(t):.2f} us per call, rounds {min(t):.2f} .. {max(t):.2f} "
                  f"({rounds} alternating rounds of {per_round} back-to-back calls, events, output allocation included)")
        g = M.design_gc_from_logits(logits, mask=m, constraints=cons, gc_content=(0.4, 0.6), **kw)
        a = D.design_count_from_logits(logits, mask=m, constraints=cons, counted=cg, window=window, cap=T, **kw)
        print("(a) against rnampnn_design_gc, hairpins: " + ", ".join(f"{k} equal {bool((x == y).all())}" for k, x, y in
                                                                    zip(("seqs", "seq_nll", "infeasible", "count", "miss"), a, g)))
        for tag, out, r in (("(b)", variants[4][1](), ref), ("(c)", variants[5][1](), ref_hp)):
            dist = ((out[0].cpu() != r[None]) & (out[0].cpu() >= 0)).sum(-1)
            print(f"{tag} mutations of the draws {int(out[3].min())} .. {int(out[3].max())} (Hamming distance equal {bool((dist == out[3].cpu()).all())}), "
                  f"mut_miss total {int(out[4].sum())}, mean NLL per nt {float(out[1].sum()) / (S * int(mask.sum())):.4f}")
    if what == "avoid":
        # Four variants in alternating rounds of one process, so that k_design_avoid is compared with k_design_count of the SAME run.
        from rnampnn.model import decode as D
        from rnampnn.utils.motifs import MotifAutomaton
        rounds, per_round, warm = 5, 10, 3
        kw = dict(temperature=0.1, seed=1)
        sets = D.mutation_sets(torch.randint(0, 4, (B, T), generator=torch.Generator().manual_seed(1)).cuda())
        run3 = MotifAutomaton.from_motifs([], max_run=3)
        wide = MotifAutomaton.from_motifs(["GGGG", "GAAUUCAAGC", "CUGCAGUCGA", "AAGCUUGCAU", "UCUAGAGGCC", "CCCGGGAUAU", "AUCGAUCGGUAC"])
        variants = [
            ("rnampnn_design_count (b) random reference, 0..8 mutations, cap 8, S 8",
             lambda: D.design_count_from_logits(logits, mask=m, counted=sets, window=(0, 8), n_samples=8, **kw)),
            (f"rnampnn_design_avoid max_run 3 ({run3.n_live} live states), S 8",
             lambda: D.design_avoid_from_logits(logits, mask=m, avoid=run3, n_samples=8, **kw)),
            (f"rnampnn_design_avoid {wide.n_states}-state set ({wide.n_live} live states), S 8",
             lambda: D.design_avoid_from_logits(logits, mask=m, avoid=wide, n_samples=8, **kw)),
            (f"rnampnn_design_avoid max_run 3 ({run3.n_live} live states), S 64",
             lambda: D.design_avoid_from_logits(logits, mask=m, avoid=run3, n_samples=64, **kw))]
        for _, fn in variants:
            for _ in range(warm):
                fn()
        torch.cuda.synchronize()
        times = [[] for _ in variants]
        for _ in range(rounds):
            for v, (_, fn) in enumerate(variants):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(per_round):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                times[v].append(e0.elapsed_time(e1) * 1e3 / per_round)
        for (name, _), t in zip(variants, times):
            print(f"B {B} T {T} nt {int(mask.sum())} {name}: {sum(t) / len(t):.2f} us per call, rounds {min(t):.2f} .. {max(t):.2f} "
                  f"({rounds} alternating rounds of {per_round} back-to-back calls, events, output allocation included)")
        free = M.design_from_logits(logits, mask=m, n_samples=8, **kw)[0]
        for tag, auto, out in (("max_run 3", run3, variants[1][1]()), ("64-state set", wide, variants[2][1]())):
            print(f"{tag}: hits of the draws {int(out[3].sum())} (recounted {int(auto.hits(out[0]).sum())}), avoid_miss total {int(out[4].sum())}, "
                  f"mean NLL per nt {float(out[1].sum()) / (8 * int(mask.sum())):.4f}; rnampnn_design's free draws hold {int(auto.hits(free).sum())} hits")
    if what == "dfa":
        # Four variants in alternating rounds of one process, so that k_design_dfa is compared with k_design_avoid of the SAME run.
        from rnampnn.model import decode as D
        from rnampnn.utils.motifs import DesignAutomaton, MotifAutomaton
        rounds, per_round, warm = 5, 10, 3
        kw = dict(temperature=0.1, seed=1, n_samples=8)
        run3 = MotifAutomaton.from_motifs([], max_run=3)
        same = DesignAutomaton(run3.delta, torch.tensor([1 if (run3.terminal >> a) & 1 else 2 for a in range(run3.n_states)], dtype=torch.uint8),
                               run3.words)
        one = DesignAutomaton.from_motifs(["GGAGG"], max_run=3)
        two = DesignAutomaton.from_motifs(["GGAGG", "CUUCG"], max_run=3)
        variants = [
            (f"rnampnn_design_avoid max_run 3 ({run3.n_live} live states), S 8", lambda: D.design_avoid_from_logits(logits, mask=m, avoid=run3, **kw)),
            (f"rnampnn_design_dfa max_run 3, every live state accepting ({same.n_live} live states), S 8",
             lambda: D.design_dfa_from_logits(logits, mask=m, require=same, **kw)),
            (f"rnampnn_design_dfa require GGAGG, max_run 3 ({one.n_states} states, {one.n_live} live), S 8",
             lambda: D.design_dfa_from_logits(logits, mask=m, require=one, **kw)),
            (f"rnampnn_design_dfa require GGAGG and CUUCG, max_run 3 ({two.n_states} states, {two.n_live} live), S 8",
             lambda: D.design_dfa_from_logits(logits, mask=m, require=two, **kw))]
        for _, fn in variants:
            for _ in range(warm):
                fn()
        torch.cuda.synchronize()
        times = [[] for _ in variants]
        for _ in range(rounds):
            for v, (_, fn) in enumerate(variants):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(per_round):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                times[v].append(e0.elapsed_time(e1) * 1e3 / per_round)
        for (name, _), t in zip(variants, times):
            print(f"B {B} T {T} nt {int(mask.sum())} {name}: {sum(t) / len(t):.2f} us per call, rounds {min(t):.2f} .. {max(t):.2f} "
                  f"({rounds} alternating rounds of {per_round} back-to-back calls, events, output allocation included)")
        a, d = variants[0][1](), variants[1][1]()
        print("every live state accepting against rnampnn_design_avoid: " + ", ".join(
            f"{k} equal {bool((x == y).all())}" for k, x, y in zip(("seqs", "seq_nll", "infeasible", "hits", "miss"), a, d[:4] + d[5:])))
        free = M.design_from_logits(logits, mask=m, **kw)[0]
        word = DesignAutomaton.from_motifs(["GGAGG"])
        for tag, auto, out in (("require GGAGG, max_run 3", one, variants[2][1]()), ("require GGAGG and CUUCG, max_run 3", two, variants[3][1]())):
            print(f"{tag}: accepted {int(out[4].sum())} of {8 * B} draws, hits {int(out[3].sum())}, dfa_miss total {int(out[5].sum())}, "
                  f"mean NLL per nt {float(out[1].sum()) / (8 * int(mask.sum())):.4f}")
        print(f"filtering yield: {int(word.scan(free)[1].sum())} of the {8 * B} free draws of rnampnn_design at temperature 0.1 contain GGAGG")
    if what == "chain":
        # Six variants in alternating rounds of one process, so that k_design_dfa_count is compared with k_design_dfa on the same automaton
        # and with k_design_count on the same windows of the SAME run.  The automaton is max_run 3 with every live state accepting.
        from rnampnn.model import decode as D
        from rnampnn.model.decode import gc_counts, gc_fractions
        from rnampnn.utils.motifs import DesignAutomaton
        import ctypes as C
        rounds, per_round, warm = 5, 10, 3
        kw = dict(temperature=0.1, seed=1, n_samples=8)
        run3 = DesignAutomaton.from_avoid([], max_run=3)
        lo, hi = gc_counts(gc_fractions((0.45, 0.60), B).cuda(), m.sum(dim=1))
        window = torch.stack([lo, hi], dim=1)
        cg = torch.full((B, T), 12, dtype=torch.uint8, device="cuda")
        ref = torch.randint(0, 4, (B, T), generator=torch.Generator().manual_seed(1)).cuda()
        sets = D.mutation_sets(ref)
        nothing, zero = torch.zeros(B, T, dtype=torch.uint8, device="cuda"), torch.zeros(B, dtype=torch.int32, device="cuda")

        def nothing_counted():                                      # the entry itself: no Python wrapper passes "nothing counts"
            def tail(B, T, m, cu):
                need = int(D._native.lib().rnampnn_design_dfa_count_workspace_bytes(B, T, run3.n_live, 1))
                return (run3.delta_on("cuda"), run3.kind, run3.n_states, nothing, zero, zero, 0,
                        torch.empty(need, dtype=torch.uint8, device="cuda"), C.c_size_t(need))
            return D._design_call("rnampnn_design_dfa_count", logits, m, None, None, 8, 0.1, 1, None, tail=tail,
                                  outputs=((torch.int32, True),) * 3 + ((torch.int32, False),) * 2 + ((torch.float64, False),))
        variants = [
            (f"rnampnn_design_dfa max_run 3, every live state accepting ({run3.n_live} live states), S 8",
             lambda: D.design_dfa_from_logits(logits, mask=m, require=run3, **kw)),
            ("rnampnn_design_count C|G counted, cap T, 45..60 %, S 8",
             lambda: D.design_count_from_logits(logits, mask=m, counted=cg, window=window, cap=T, **kw)),
            ("rnampnn_design_count random reference, 0..8 mutations, cap 8, S 8",
             lambda: D.design_count_from_logits(logits, mask=m, counted=sets, window=(0, 8), **kw)),
            ("rnampnn_design_dfa_count max_run 3, nothing counted, cap 0, S 8", nothing_counted),
            ("rnampnn_design_dfa_count max_run 3, G+C 45..60 %, cap T, S 8",
             lambda: D.design_dfa_count_from_logits(logits, mask=m, require=run3, gc_content=(0.45, 0.60), **kw)),
            ("rnampnn_design_dfa_count max_run 3, 0..8 mutations, cap 8, S 8",
             lambda: D.design_dfa_count_from_logits(logits, mask=m, require=run3, mutations=(ref, (0, 8)), **kw))]
        for _, fn in variants:
            for _ in range(warm):
                fn()
        torch.cuda.synchronize()
        times = [[] for _ in variants]
        for _ in range(rounds):
            for v, (_, fn) in enumerate(variants):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(per_round):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                times[v].append(e0.elapsed_time(e1) * 1e3 / per_round)
        for (name, _), t in zip(variants, times):
            print(f"B {B} T {T} nt {int(mask.sum())} {name}: {sum(t) / len(t):.2f} us per call, rounds {min(t):.2f} .. {max(t):.2f} "
                  f"({rounds} alternating rounds of {per_round} back-to-back calls, events, output and workspace allocation included)")
        a, d = variants[0][1](), variants[3][1]()
        print("nothing counted against rnampnn_design_dfa: " + ", ".join(
            f"{k} equal {bool((x == y).all())}" for k, x, y in zip(("seqs", "seq_nll", "infeasible", "hits", "accepted", "dfa_miss"), a, d[:5] + d[6:7])))
        n = m.sum(dim=1)
        for tag, out, within in (("G+C 45..60 %", variants[4][1](), lambda c: (c >= lo[None]) & (c <= hi[None])),
                                 ("0..8 mutations", variants[5][1](), lambda c: c <= 8)):
            q = out[0]
            recount = ((q == 2) | (q == 3)).sum(-1) if tag.startswith("G+C") else ((q != ref[None]) & (q >= 0)).sum(-1)
            print(f"{tag}: accepted {int(out[4].sum())} of {8 * B} draws, hits {int(out[3].sum())} (recounted {int(run3.scan(q)[0].sum())}), "
                  f"count inside the window {int(within(out[5]).sum())} of {8 * B} (recount equal {bool((recount == out[5]).all())}), dfa_miss total "
                  f"{int(out[6].sum())}, count_miss total {int(out[7].sum())}, mean NLL per nt {float(out[1].sum()) / (8 * int(mask.sum())):.4f}")
        ws = [int(D._native.lib().rnampnn_design_dfa_count_workspace_bytes(B, T, run3.n_live, cap)) for cap in (1, 8, T)]
        print(f"workspace at (B {B}, T {T}, {run3.n_live} live states): {ws[0] // 2} bytes at cap 0, {ws[1]} at cap 8, {ws[2]} at cap T")
    if what == "nested":
        # Four variants in alternating rounds of one process, so that k_design_nested is compared with k_design_dfa of the SAME run.  The
        # structure: three outer pairs around a multiloop of hairpins (a stem of 4 closed by a tetraloop, 2 unpaired between them).
        from rnampnn.model import decode as D
        from rnampnn.utils.motifs import DesignAutomaton
        rounds, per_round, warm = 5, 10, 3
        kw = dict(temperature=0.1, seed=1, n_samples=8)
        run3 = DesignAutomaton.from_avoid([], max_run=3)
        gnra = DesignAutomaton.from_motifs(["GNRA"], max_run=3)
        rich = []
        for n in lens:
            k = (n - 8) // 14
            body = ("((((....))))" + "..") * k
            rich.append((None, "(((" + "." + body + "." * (n - 8 - 14 * k) + "." + ")))"))
        nest = DesignConstraints.from_specs(rich, lens, T).to_device("cuda")
        n_pairs = int((nest.partner >= 0).sum()) // 2
        variants = [
            (f"rnampnn_design_dfa max_run 3, every live state accepting ({run3.n_live} live states), no pairs, S 8",
             lambda: D.design_dfa_from_logits(logits, mask=m, require=run3, **kw)),
            (f"rnampnn_design_nested max_run 3 ({run3.n_live} live states), no pairs, S 8",
             lambda: D.design_nested_from_logits(logits, mask=m, require=run3, **kw)),
            (f"rnampnn_design_nested max_run 3 ({run3.n_live} live states), {n_pairs} nested pairs in the batch, S 8",
             lambda: D.design_nested_from_logits(logits, mask=m, require=run3, constraints=nest, **kw)),
            (f"rnampnn_design_nested require GNRA, max_run 3 ({gnra.n_states} states, {gnra.n_live} live), {n_pairs} nested pairs in the batch, S 8",
             lambda: D.design_nested_from_logits(logits, mask=m, require=gnra, constraints=nest, **kw))]
        for _, fn in variants:
            for _ in range(warm):
                fn()
        torch.cuda.synchronize()
        times = [[] for _ in variants]
        for _ in range(rounds):
            for v, (_, fn) in enumerate(variants):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(per_round):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                times[v].append(e0.elapsed_time(e1) * 1e3 / per_round)
        for (name, _), t in zip(variants, times):
            print(f"B {B} T {T} nt {int(mask.sum())} {name}: {sum(t) / len(t):.2f} us per call, rounds {min(t):.2f} .. {max(t):.2f} "
                  f"({rounds} alternating rounds of {per_round} back-to-back calls, events, output and workspace allocation included)")
        a, d = variants[0][1](), variants[1][1]()
        print("no pairs against rnampnn_design_dfa: " + ", ".join(
            f"{k} equal {bool((x == y).all())}" for k, x, y in zip(("seqs", "seq_nll", "infeasible", "hits", "accepted", "dfa_miss"), a, d)))
        pa = nest.partner.cpu()
        for tag, auto, out in (("max_run 3 under the structure", run3, variants[2][1]()), ("require GNRA, max_run 3 under the structure", gnra, variants[3][1]())):
            q = out[0].cpu()
            lo = (pa >= 0) & (pa > torch.arange(T)[None])
            left, right = q[:, lo], torch.gather(q, 2, pa.clamp(min=0).to(torch.int64)[None].expand(q.shape[0], -1, -1))[:, lo]
            ok = ((left == 0) & (right == 1)) | ((left == 1) & ((right == 0) | (right == 3))) | ((left == 2) & (right == 3)) | ((left == 3) & ((right == 2) | (right == 1)))
            print(f"{tag}: accepted {int(out[4].sum())} of {8 * B} draws, hits {int(out[3].sum())} (recounted {int(auto.scan(out[0])[0].sum())}), "
                  f"dfa_miss total {int(out[5].sum())}, nest_miss total {int(out[6].sum())}, compatible pairs {int(ok.sum())} of {ok.numel()}, "
                  f"mean NLL per nt {float(out[1].sum()) / (8 * int(mask.sum())):.4f}")
        ws = [int(D._native.lib().rnampnn_design_nested_workspace_bytes(B, T, a.n_live)) for a in (run3, gnra)]
        print(f"workspace at (B {B}, T {T}): {ws[0]} bytes at {run3.n_live} live states, {ws[1]} bytes at {gnra.n_live}")
    if what == "profile":
        # Seven variants in alternating rounds of one process: the two draw kernels the profiles share their tables with, then the profiles.
        from rnampnn.model import decode as D
        from rnampnn.utils.motifs import MotifAutomaton
        rounds, per_round, warm = 5, 10, 3
        ref = torch.randint(0, 4, (B, T), generator=torch.Generator().manual_seed(1)).cuda()
        sets = D.mutation_sets(ref)
        run3 = MotifAutomaton.from_motifs([], max_run=3)
        wide = MotifAutomaton.from_motifs(["GGGG", "GAAUUCAAGC", "CUGCAGUCGA", "AAGCUUGCAU", "UCUAGAGGCC", "CCCGGGAUAU", "AUCGAUCGGUAC"])
        pk = dict(mask=m, temperature=0.1)
        variants = [
            ("rnampnn_design_count (b) random reference, 0..8 mutations, cap 8, S 8",
             lambda: D.design_count_from_logits(logits, mask=m, counted=sets, window=(0, 8), n_samples=8, temperature=0.1, seed=1)),
            (f"rnampnn_design_avoid max_run 3 ({run3.n_live} live states), S 8",
             lambda: D.design_avoid_from_logits(logits, mask=m, avoid=run3, n_samples=8, temperature=0.1, seed=1)),
            ("rnampnn_design_count_profile G+C 40..60 %, cap T, no constraints", lambda: D.design_profile_from_logits(logits, gc_content=(0.4, 0.6), **pk)),
            ("rnampnn_design_count_profile 0..8 mutations, cap 8, no constraints", lambda: D.design_profile_from_logits(logits, mutations=(ref, 8), **pk)),
            ("rnampnn_design_count_profile plain, cap 0, hairpin pairs + GNRA + bias", lambda: D.design_profile_from_logits(logits, constraints=cons, **pk)),
            (f"rnampnn_design_avoid_profile max_run 3 ({run3.n_live} live states)", lambda: D.design_profile_from_logits(logits, avoid=run3, **pk)),
            (f"rnampnn_design_avoid_profile {wide.n_states}-state set ({wide.n_live} live states)",
             lambda: D.design_profile_from_logits(logits, avoid=wide, **pk))]
        for _, fn in variants:
            for _ in range(warm):
                fn()
        torch.cuda.synchronize()
        times = [[] for _ in variants]
        for _ in range(rounds):
            for v, (_, fn) in enumerate(variants):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(per_round):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                times[v].append(e0.elapsed_time(e1) * 1e3 / per_round)
        for (name, _), t in zip(variants, times):
            print(f"B {B} T {T} nt {int(mask.sum())} {name}: {sum(t) / len(t):.2f} us per call, rounds {min(t):.2f} .. {max(t):.2f} "
                  f"({rounds} alternating rounds of {per_round} back-to-back calls, events, output allocation included)")
        for (name, fn) in variants[2:]:
            p = fn()
            rows = p.marginals.sum(-1)
            print(f"{name.split(',')[0]}: log_mass {float(p.log_mass.min()):.3f} .. {float(p.log_mass.max()):.3f} nats, entropy "
                  f"{float(p.entropy.min()):.3f} .. {float(p.entropy.max()):.3f} nats, miss total {int(p.miss.sum())}, "
                  f"max |row sum - 1| on valid positions {float(((rows - 1).abs() * m).max()):.2e}")
    if what == "dfa_profile":
        # Seven variants in alternating rounds of one process: rnampnn_design_dfa (S = 8) at three automata and rnampnn_design_avoid_profile
        # at the one it knows - the yardsticks of the same run - then rnampnn_design_dfa_profile at the three; then one RNA at the largest T.
        from rnampnn.model import decode as D
        from rnampnn.utils.motifs import DesignAutomaton, MotifAutomaton
        rounds, per_round, warm = 5, 10, 3
        long_word = "GGAGGCUUCGAAUUCGCAUGCCAUGGUACCUAGCUAGGAUCCGAUAUCAAGCUUGCGGCCGCUCGAGACGUCUGCAGCCCGGGAGAUCUGUCGACACUAGUUCUAGA"
        run3 = MotifAutomaton.from_motifs([], max_run=3)
        autos = [("max_run 3", DesignAutomaton.from_avoid(run3)), ("require GGAGG and CUUCG, max_run 3", DesignAutomaton.from_motifs(["GGAGG", "CUUCG"], max_run=3)),
                 ("require a 26-mer and a 39-mer", DesignAutomaton.from_motifs([long_word[:26], long_word[50:89]]))]
        kw = dict(temperature=0.1, seed=1, n_samples=8)
        pk = dict(mask=m, temperature=0.1)
        variants = [(f"rnampnn_design_dfa {tag} ({a.n_states} states, {a.n_live} live), S 8",
                     lambda a=a: D.design_dfa_from_logits(logits, mask=m, require=a, **kw)) for tag, a in autos]
        variants.append((f"rnampnn_design_avoid_profile max_run 3 ({run3.n_live} live states)", lambda: D.design_profile_from_logits(logits, avoid=run3, **pk)))
        variants += [(f"rnampnn_design_dfa_profile {tag} ({a.n_states} states, {a.n_live} live)",
                      lambda a=a: D.design_profile_from_logits(logits, require=a, table="global", **pk)) for tag, a in autos]
        for _, fn in variants:
            for _ in range(warm):
                fn()
        torch.cuda.synchronize()
        times = [[] for _ in variants]
        for _ in range(rounds):
            for v, (_, fn) in enumerate(variants):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(per_round):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                times[v].append(e0.elapsed_time(e1) * 1e3 / per_round)
        for (name, _), t in zip(variants, times):
            print(f"B {B} T {T} nt {int(mask.sum())} {name}: {sum(t) / len(t):.2f} us per call, rounds {min(t):.2f} .. {max(t):.2f} "
                  f"({rounds} alternating rounds of {per_round} back-to-back calls, events, output allocation included)")
        t_max = 4498                                                # the largest T the entry accepts (include/rnampnn_hip.h)
        one = (3.0 * torch.randn(1, t_max, 4, generator=torch.Generator().manual_seed(2))).cuda()
        ones = torch.ones(1, t_max, device="cuda")
        big = lambda: D.design_profile_from_logits(one, mask=ones, temperature=0.1, require=autos[0][1], table="global")
        for _ in range(warm):
            big()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(per_round):
            big()
        e1.record()
        torch.cuda.synchronize()
        print(f"B 1 T {t_max} rnampnn_design_dfa_profile max_run 3 ({autos[0][1].n_live} live states): {e0.elapsed_time(e1) * 1e3 / per_round:.2f} us per call "
              f"({per_round} back-to-back calls, events, output allocation included)")
        for (name, fn) in variants[3:] + [("rnampnn_design_dfa_profile one RNA of 4498 nt", big)]:
            p = fn()
            rows, valid = p.marginals.sum(-1), (m if p.marginals.shape[0] == B else ones)
            print(f"{name.split('(')[0].strip()}: log_mass {float(p.log_mass.min()):.3f} .. {float(p.log_mass.max()):.3f} nats, entropy "
                  f"{float(p.entropy.min()):.3f} .. {float(p.entropy.max()):.3f} nats, miss total {int(p.miss.sum())}, "
                  f"max |row sum - 1| on valid positions {float(((rows - 1).abs() * valid).max()):.2e}")
        a, p = variants[3][1](), variants[4][1]()
        print(f"max_run 3, the two homes of the table: max |dP| {float((a.marginals - p.marginals).abs().max()):.2e}, max |d log_z| "
              f"{float((a.log_z - p.log_z).abs().max()):.2e}, max |d entropy| {float((a.entropy - p.entropy).abs().max()):.2e}")
    if what == "distinct":
        for S in (8, 64):                                           # (timed() prints the global S)
            for mode in ("sample", "best"):
                kw = dict(n_samples=S, temperature=0.1, seed=1, mode=mode)
                timed(f"rnampnn_design_distinct {mode}, no constraints", lambda: M.design_distinct_from_logits(logits, mask=m, **kw))
                timed(f"rnampnn_design_distinct {mode}, hairpin pairs + GNRA + bias",
                      lambda: M.design_distinct_from_logits(logits, mask=m, constraints=cons, **kw))
            d_seqs, d_nll, d_bad, d_logp, d_n = M.design_distinct_from_logits(logits, mask=m, n_samples=S, temperature=0.1, seed=1, mode="sample")
            dup = sum(S - len({r.tobytes() for r in q.cpu().numpy()})
                      for q in M.design_from_logits(logits, mask=m, n_samples=S, temperature=0.1, seed=1)[0].permute(1, 0, 2))
            print(f"S {S}: slots filled {int(d_n.min())} .. {int(d_n.max())}, total probability of an RNA's {S} distinct designs "
                  f"{float(d_logp.double().exp().sum(0).min()):.4f} .. {float(d_logp.double().exp().sum(0).max()):.4f}; of rnampnn_design's "
                  f"{S * B} independent free draws at the same temperature {dup} repeat an earlier draw of their RNA")
    if what == "tied":
        one = [1] * B
        timed("rnampnn_design_tied, one state per group, no constraints",
              lambda: M.design_from_logits(logits, mask=m, n_samples=S, temperature=0.1, seed=1, states=one))
        timed("rnampnn_design_tied, one state per group, hairpin pairs + GNRA + bias",
              lambda: M.design_from_logits(logits, mask=m, n_samples=S, temperature=0.1, seed=1, constraints=cons, states=one))
        t_seqs, t_nll, t_bad = M.design_from_logits(logits, mask=m, n_samples=S, temperature=0.1, seed=1, constraints=cons, states=one)
        print(f"one state per group against rnampnn_design: {int((t_seqs != seqs).sum())} of {S * int(mask.sum())} ids differ, "
              f"infeasible equal {bool((t_bad == bad).all())}")
        # 64 groups x 4 states (conformers of one length); states 0 and 1 share position n // 2: the 3-node chain 5 - n // 2 - n - 6
        lens4 = [lens[g] for g in range(B // 4) for _ in range(4)]
        m4 = torch.zeros(B, T)
        partner = np.full((B, T), -1, dtype=np.int32)
        for b, n in enumerate(lens4):
            m4[b, :n] = 1
            if b % 4 == 0:
                partner[b, 5], partner[b, n // 2] = n // 2, 5
            if b % 4 == 1:
                partner[b, n // 2], partner[b, n - 6] = n - 6, n // 2
        m4 = m4.cuda()
        logits4 = logits * m4[..., None]
        cons4 = DesignConstraints(None, torch.from_numpy(partner), None, True).to_device("cuda")
        four = [4] * (B // 4)
        timed("rnampnn_design_tied, 64 groups x 4 states, one 3-node chain per group",
              lambda: M.design_from_logits(logits4, mask=m4, n_samples=S, temperature=0.1, seed=1, constraints=cons4, states=four))
        q, _, bad4 = M.design_from_logits(logits4, mask=m4, n_samples=S, temperature=0.1, seed=1, constraints=cons4, states=four)
        print(f"64 x 4: infeasible positions {int(bad4.sum())}, rows of a group identical {bool((q.view(S, B // 4, 4, T) == q.view(S, B // 4, 4, T)[:, :, :1]).all())}")
