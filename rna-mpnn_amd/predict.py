#!/usr/bin/env python3
"""Design sequences for a directory of structures with a trained model - the role of the reference's ``main.py:17-31``:

    python rna-mpnn_amd/predict.py --ckpt runs/rnampnn/Final.pt [--xgb runs/rnampnn/XGB.json] --data /path/to/data --out submit.csv
    python rna-mpnn_amd/predict.py --ckpt runs/rnampnn/Final.pt --data /path/to/data --samples 8 --temperature 0.1 --designs-out designs.csv

``--ckpt`` is what ``train.py --out DIR`` wrote (weights + constructor arguments, loaded with ``weights_only=True``; pickles are never
loaded).  Its ``model`` key chooses the family: ``"rnampnn"`` = ``RNAMPNN``; a file without the key is an ``rdesign`` checkpoint (the files
``train.py --model rdesign`` has always written).  ``--xgb`` is the tree read-out in XGBoost's JSON schema - without it the read-out's argmax
decides, as in the reference with an unfitted XGBoost head.  ``--data`` holds ``coords/<id>.npy`` (L,7,3) and ``seqs/<id>.fasta`` (optional for
``RNAMPNN``); the CSV has one ``pdb_id,seq`` row per structure in id order.  ``--samples N`` also draws N sequences per structure at
``--temperature`` and writes them with their per-nucleotide NLL and recovery to ``--designs-out``.

    python rna-mpnn_amd/predict.py --ckpt Final.pt --data DIR --samples 8 --constraints cons.csv --bias G=-0.5 --omit "" --no-wobble

Constrained design (``rnampnn_design``, one launch on the packed logits): ``--constraints`` is a CSV ``pdb_id,fixed,structure`` - ``fixed`` a
pattern of AUCG / IUPAC codes with ``.`` or ``-`` for free positions, ``structure`` a dot-bracket string whose pairs are drawn together as
AU UA GC CG (GU UG unless ``--no-wobble``); either may be empty and ids not listed are unconstrained.  ``--bias A=..,U=..,C=..,G=..`` is added
to the logits, ``--omit LETTERS`` never draws these letters.  With any of the four the designs CSV gains the column ``infeasible`` (positions
whose constraint could not be honoured).

    python rna-mpnn_amd/predict.py --ckpt Final.pt --data DIR --samples 8 --states states.csv [--constraints cons.csv]

Multi-state design (``rnampnn_design_tied``, ``rnampnn`` checkpoints): ``--states`` is a CSV ``design_id,pdb_id,weight`` - the structures
listed under one ``design_id`` (conformers of an ensemble, the two backbones of a switch) are the states of ONE design and receive the same
sequence, drawn from the product of their distributions; ``weight`` may be empty (1) or negative (design against that state); structures
not listed are designs of their own.  ``--constraints`` rows still go by ``pdb_id``, so each state brings its own structure, and the one
sequence is pair-compatible in all of them.  The designs CSV then has one row per (design, sample):
``design_id,sample,seq,infeasible,states,nll_per_nt,recovery``, the last three ``;``-joined per state.

    python rna-mpnn_amd/predict.py --ckpt Final.pt --data DIR --samples 8 --gc-content 0.45:0.60 [--constraints cons.csv --bias .. --omit .. --no-wobble]

G+C content window (``rnampnn_design_gc``, both families): every draw holds a fraction of C and G between LO and HI of its length - drawn
exactly from the model's distribution conditioned on that (and on the other constraints), not filtered.  The designs CSV gains the columns
``gc`` (the fraction of the draw) and ``gc_miss`` (0, or by how many nucleotides the nearest count the constraints can reach lies outside
the window; the draws then hold that count).  Not built together with ``--states``.  The count tree of the window lives in the LDS of a
workgroup, which holds structures of up to 1,017 nt (2,867 for ``--max-mutations 8``); ``--tree global`` keeps it in a workspace in global
memory instead (``rnampnn_design_count_long``, up to 32,744 nt - a ribosomal RNA), ``--tree auto`` does so where LDS refuses.  The draws
are the same bytes wherever both run.  ``--tree global`` / ``auto`` with a mode that has no count tree is refused before the checkpoint is
opened.

    python rna-mpnn_amd/predict.py --ckpt Final.pt --data DIR --samples 8 --distinct sample [--constraints cons.csv --bias .. --omit .. --no-wobble]

Distinct designs (``rnampnn_design_distinct``, both families, at most 256 per structure): the N sequences of a structure are pairwise
different - ``sample`` draws them without replacement from the model's (constrained, tempered) distribution, ``best`` lists its N most
probable sequences in descending order.  The designs CSV gains a last column ``logp`` (the log-probability of the sequence under that
distribution); a structure that admits fewer than N sequences has fewer rows.  Not built together with ``--states`` or ``--gc-content``.

    python rna-mpnn_amd/predict.py --ckpt Final.pt --data DIR --samples 8 --max-mutations 6 [--min-mutations 2] [--mutate-from parents.fasta]

Mutation budget (``rnampnn_design_count``, both families): every draw differs from the structure's reference sequence at no more than M
(and no fewer than m) positions - drawn exactly from the model's distribution conditioned on that and on the other constraints, not
filtered.  The reference is the structure's own ``seqs/<id>.fasta``, or its record ``>pdb_id`` in ``--mutate-from`` (letters outside AUCG
never count); a structure without one is an error naming its id.  The designs CSV gains the columns ``mutations`` (the Hamming distance of
the draw to the reference) and ``mut_miss`` (0, or by how many mutations the target structure and the fixed positions alone exceed the
budget; the draws then hold the fewest mutations they allow).  Not built together with ``--states``, ``--gc-content`` or ``--distinct``.

    python rna-mpnn_amd/predict.py --ckpt Final.pt --data DIR --samples 8 --avoid GGGG,GAAUUC [--max-run 3] [--constraints cons.csv --bias .. --omit ..]

Forbidden motifs (``rnampnn_design_avoid``, both families): no draw contains one of the comma-separated motifs (AUCG, T read as U, IUPAC
codes expand) or, with ``--max-run R``, a run of more than R equal letters - drawn exactly from the model's distribution conditioned on
that and on the fixed positions, not filtered.  The designs CSV gains the columns ``motif_hits`` (positions of the draw at which a motif
ends) and ``avoid_miss`` (1 for a structure whose fixed positions spell a motif: its draws ignore the motifs and ``motif_hits`` reports
them).  Not built together with the other modes or with a ``structure`` in ``--constraints``; the automaton of the set has at most 64
states.

    python rna-mpnn_amd/predict.py --ckpt Final.pt --data DIR --samples 8 --require GGAGG,GNRA [--avoid GAAUUC] [--max-run 3] [--constraints cons.csv ..]

Required motifs (``rnampnn_design_dfa``, both families): every draw contains EVERY one of the comma-separated motifs somewhere (any expansion
of an IUPAC motif counts) and none of ``--avoid`` / ``--max-run`` - drawn exactly from the model's distribution conditioned on that and on
the fixed positions, not filtered.  The designs CSV gains the columns ``motif_hits``, ``required_found`` (1 when the draw holds every
required motif) and ``require_miss`` (1 for a structure that cannot hold them: its draws ignore the motifs).  Not built together with the
other modes, ``--profile-out`` or a ``structure`` in ``--constraints``; the automaton has at most 256 states and 6 required motifs.

    python rna-mpnn_amd/predict.py --ckpt Final.pt --data DIR --samples 8 --pairs nested --constraints cons.csv [--avoid GGGG] [--max-run 3] [--require GNRA]

Motifs under base pairs (``rnampnn_design_nested``, both families): ``--pairs nested`` lifts the refusal of a ``structure`` in
``--constraints`` for ``--avoid``, ``--max-run`` and ``--require``: the draws pair as the structure says AND hold the motif conditions,
drawn exactly from the model's distribution conditioned on both.  The structures must be nested: one with a pseudoknot is an error naming
its ids, before the checkpoint is opened.  The designs CSV gains the columns ``motif_hits``, ``required_found``, ``require_miss`` and
``nest_miss``.  At most 64 live automaton states; not built together with the other modes or ``--profile-out``.

    python rna-mpnn_amd/predict.py --ckpt Final.pt --data DIR --samples 8 --combine chain --avoid GGGG,GAAUUC --max-run 3 --require GNRA --gc-content 0.45:0.60
    python rna-mpnn_amd/predict.py --ckpt Final.pt --data DIR --samples 8 --combine chain --avoid GAAUUC --max-mutations 6 [--min-mutations 2] [--mutate-from parents.fasta]

Motifs under a count window (``rnampnn_design_dfa_count``, both families): ``--combine chain`` lifts the refusal of ``--avoid`` /
``--max-run`` / ``--require`` together with ``--gc-content`` or ``--max-mutations``: every draw holds the motif conditions AND its G+C
content lies in the window (or it differs from its reference within the budget), drawn exactly from the model's distribution conditioned on
both - an oligo to order, not a filtered sample.  The designs CSV gains the columns ``motif_hits``, ``required_found``, ``require_miss`` and
then ``gc_count``, ``gc_miss`` (absolute counts) or ``mutations``, ``mut_miss``.  Needs a motif flag and exactly one of the two counts; not
built together with ``--states``, ``--distinct``, ``--pairs``, ``--tree global`` / ``auto``, ``--profile-out`` or a ``structure`` in
``--constraints``; all of that is refused before the checkpoint is opened.

    python rna-mpnn_amd/predict.py --ckpt Final.pt --data DIR --profile-out PREFIX [--gc-content .. | --max-mutations .. | --avoid ..] [--samples 8]

Design profiles (``rnampnn_design_count_profile`` / ``rnampnn_design_avoid_profile``, both families): what the draws of the chosen mode come
FROM - the exact distribution under ``--temperature``, ``--constraints``, ``--bias``, ``--omit``, ``--no-wobble`` and the mode's own flags,
computed, not estimated from samples, with or without ``--samples``.  ``PREFIX.positions.csv`` has one row per nucleotide,
``pdb_id,position,pA,pU,pC,pG`` (position 1-based; a sequence logo, a bias for another tool); ``PREFIX.rnas.csv`` one row per structure,
``pdb_id,length,log_mass,entropy,infeasible,miss``: ``log_mass`` <= 0 is the log of the share of the model's mass the constraints keep,
``entropy`` (nats) how diverse the designs can be, ``miss`` the mode's ``gc_miss`` / ``mut_miss`` / ``avoid_miss``.  Not built together with
``--states`` or ``--distinct``.

    python rna-mpnn_amd/predict.py --ckpt Final.pt --data DIR --profile-out PREFIX --table global [--require GGAGG,GNRA] [--avoid ..] [--max-run 3] [--samples 8]

Profiles under required motifs (``rnampnn_design_dfa_profile``, both families): ``--table global`` lifts the refusal of ``--require``
together with ``--profile-out`` - where the motif will land and whether ``log_mass`` is e^-2 or e^-100, computed on the automaton of up to
256 states with its table in global memory (structures of up to 4498 nt).  It serves ``--avoid`` / ``--max-run`` alone as well; the files
keep their columns and ``miss`` holds ``dfa_miss``.  Needs ``--profile-out`` and a motif flag; not built together with another mode."""
from __future__ import annotations

import argparse
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)


def parse(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--ckpt", required=True)
    ap.add_argument("--xgb", default=None)
    ap.add_argument("--data", required=True)
    ap.add_argument("--out", default="submit.csv")
    ap.add_argument("--batch-size", type=int, default=32)
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--samples", type=int, default=0, help="sequences drawn per structure (0 = none)")
    ap.add_argument("--temperature", type=float, default=0.1, help="sampling temperature of --samples")
    ap.add_argument("--seed", type=int, default=0, help="seed of --samples")
    ap.add_argument("--designs-out", default=None, help="CSV of the sampled designs (default: <out>_designs.csv)")
    ap.add_argument("--constraints", default=None, help="CSV pdb_id,fixed,structure: sequence pattern and dot-bracket structure per id")
    ap.add_argument("--bias", default=None, help="A=..,U=..,C=..,G=..: added to the logits of --samples")
    ap.add_argument("--omit", default="", help="letters --samples never draws")
    ap.add_argument("--no-wobble", action="store_true", help="base pairs of --constraints exclude GU / UG")
    ap.add_argument("--states", default=None, help="CSV design_id,pdb_id,weight: the structures of one design_id share one sequence")
    ap.add_argument("--gc-content", default=None, help="LO:HI: every draw of --samples holds a G+C fraction in this window")
    ap.add_argument("--tree", default=None, choices=("lds", "global", "auto"),
                    help="where the count tree of --gc-content / --max-mutations lives: lds (the default, structures of up to 1017 nt under a G+C "
                         "window), global (a workspace in global memory, up to 32744 nt) or auto (lds where it fits); the draws are the same")
    ap.add_argument("--distinct", default=None, choices=("sample", "best"),
                    help="the draws of --samples are pairwise different: sampled without replacement, or the most probable ones")
    ap.add_argument("--max-mutations", type=int, default=None, help="M: every draw of --samples differs from its reference at no more than M positions")
    ap.add_argument("--min-mutations", type=int, default=None, help="m: ... and at no fewer than m positions (default 0); needs --max-mutations")
    ap.add_argument("--mutate-from", default=None, help="FASTA with one record >pdb_id per structure: the references of --max-mutations "
                                                        "(default: the structure's own sequence)")
    ap.add_argument("--avoid", default=None, help="MOTIF[,MOTIF..]: no draw of --samples contains one of these substrings (AUCG, T = U, IUPAC codes)")
    ap.add_argument("--max-run", type=int, default=None, help="R: no draw of --samples holds a run of more than R equal letters")
    ap.add_argument("--require", default=None, help="MOTIF[,MOTIF..]: every draw of --samples contains every one of these substrings somewhere "
                                                    "(AUCG, T = U, IUPAC codes); usable with --avoid / --max-run")
    ap.add_argument("--pairs", default=None, choices=("nested",),
                    help="nested: --avoid / --max-run / --require hold UNDER the structures of --constraints (which must be free of pseudoknots)")
    ap.add_argument("--combine", default=None, choices=("chain",),
                    help="chain: --avoid / --max-run / --require hold TOGETHER with --gc-content or --max-mutations, exactly in both")
    ap.add_argument("--profile-out", default=None, help="PREFIX: write the exact distribution the draws come from to PREFIX.positions.csv "
                                                        "(per-position marginals) and PREFIX.rnas.csv (log_mass, entropy)")
    ap.add_argument("--table", default=None, choices=("lds", "global"),
                    help="where the table of the --profile-out of --avoid / --max-run / --require lives: lds (the default: forbidden motifs "
                         "alone, at most 64 states) or global (a workspace in global memory: required motifs too, up to 256 states, 4498 nt)")
    return ap.parse_args(argv)


def design_options(args) -> dict:
    """The constrained-design keywords of ``predict`` from the flags; empty when none of them is given."""
    if not (args.constraints or args.bias or args.omit or args.no_wobble):
        return {}
    from rnampnn.utils.constraints import omit_mask, parse_bias, read_constraints_csv
    omit_mask(args.omit)                                           # a letter outside AUCG fails here, before the model is loaded
    return dict(constraints=read_constraints_csv(args.constraints) if args.constraints else None,
                bias=parse_bias(args.bias) if args.bias else None, omit=args.omit, wobble=not args.no_wobble)


def gc_option(args) -> dict:
    """The ``gc_content`` keyword of ``predict`` from ``--gc-content``; empty without the flag.  ``ValueError`` naming the flags for a
    malformed window, with ``--states`` and without ``--samples``."""
    if args.gc_content is None:
        return {}
    from rnampnn.utils.constraints import parse_gc_content
    if args.states:
        raise ValueError("--gc-content together with --states is not built: the G+C window conditions single-state designs only")
    if args.samples <= 0 and not args.profile_out:
        raise ValueError("--gc-content needs --samples N > 0")
    return dict(gc_content=parse_gc_content(args.gc_content))


def tree_option(args) -> dict:
    """The ``tree`` keyword of ``predict`` from ``--tree``; empty without the flag.  ``ValueError`` naming the flags for ``global`` / ``auto``
    with a mode that has no count tree, before the checkpoint is opened."""
    if args.tree is None:
        return {}
    for flag, value in (("--pairs", args.pairs), ("--states", args.states), ("--distinct", args.distinct), ("--require", args.require),
                        ("--avoid", args.avoid), ("--max-run", args.max_run)):
        if value is not None and args.tree != "lds":
            raise ValueError(f"--tree {args.tree} together with {flag} is not built: only the count tree of --gc-content and --max-mutations has "
                             "a home in global memory")
    if args.tree != "lds" and args.gc_content is None and args.max_mutations is None and (args.samples > 0 or not args.profile_out):
        raise ValueError(f"--tree {args.tree} needs --gc-content or --max-mutations: a draw without a count window has no count tree")
    return dict(tree=args.tree)


def distinct_option(args) -> dict:
    """The ``distinct`` keyword of ``predict`` from ``--distinct``; empty without the flag.  ``ValueError`` naming the flags with ``--states``
    or ``--gc-content`` and without ``--samples``."""
    if args.distinct is None:
        return {}
    for flag, value in (("--states", args.states), ("--gc-content", args.gc_content)):
        if value:
            raise ValueError(f"--distinct together with {flag} is not built: distinct designs are single-state and have no G+C window")
    if args.samples <= 0:
        raise ValueError("--distinct needs --samples N > 0")
    return dict(distinct=args.distinct)


def mutations_option(args) -> dict:
    """The ``mutations`` keyword of ``predict`` from ``--max-mutations`` / ``--min-mutations`` / ``--mutate-from``; empty without them.
    ``ValueError`` naming the flags for a budget that is not 0 <= m <= M, one of the other two flags without ``--max-mutations``, with
    ``--states``, ``--gc-content`` or ``--distinct`` and without ``--samples``."""
    if args.max_mutations is None:
        if args.min_mutations is not None or args.mutate_from:
            raise ValueError("--min-mutations and --mutate-from need --max-mutations M")
        return {}
    for flag, value in (("--states", args.states), ("--gc-content", args.gc_content), ("--distinct", args.distinct)):
        if value:
            raise ValueError(f"--max-mutations together with {flag} is not built: the budget conditions plain single-state designs only")
    lo = 0 if args.min_mutations is None else args.min_mutations
    if lo < 0 or args.max_mutations < lo:
        raise ValueError(f"--max-mutations / --min-mutations: the budget needs 0 <= m <= M, got m = {lo}, M = {args.max_mutations}")
    if args.samples <= 0 and not args.profile_out:
        raise ValueError("--max-mutations needs --samples N > 0")
    from rnampnn.utils.constraints import read_reference_fasta
    return dict(mutations=(lo, args.max_mutations, read_reference_fasta(args.mutate_from) if args.mutate_from else None))


def avoid_option(args) -> dict:
    """The ``avoid`` keyword of ``predict`` from ``--avoid`` / ``--max-run``: the automaton, built (and refused) before the model is loaded;
    empty without the flags.  ``ValueError`` naming the flags with another mode and without ``--samples``."""
    if (args.avoid is None and args.max_run is None) or args.require is not None:
        return {}                                                  # (--require takes both into its own automaton: require_option)
    for flag, value in (("--states", args.states), ("--gc-content", args.gc_content), ("--distinct", args.distinct),
                        ("--max-mutations", args.max_mutations)):
        if value is not None:
            raise ValueError(f"--avoid / --max-run together with {flag} is not built: the automaton conditions plain single-state designs only")
    if args.samples <= 0 and not args.profile_out:
        raise ValueError("--avoid / --max-run need --samples N > 0")
    from rnampnn.utils.motifs import MotifAutomaton
    return dict(avoid=MotifAutomaton.from_motifs([m for m in (args.avoid or "").split(",") if m.strip()], max_run=args.max_run))


def require_option(args) -> dict:
    """The ``require`` keyword of ``predict`` from ``--require`` with ``--avoid`` / ``--max-run``: one automaton of both lists, built (and
    refused) before the model is loaded; empty without ``--require``.  ``ValueError`` naming the flags with another mode or
    ``--profile-out`` and without ``--samples``."""
    if args.require is None:
        return {}
    profiled = args.table == "global" and args.profile_out is not None          # --table global: the profile of rnampnn_design_dfa_profile
    for flag, value in (("--profile-out", None if profiled else args.profile_out), ("--states", args.states), ("--gc-content", args.gc_content),
                        ("--distinct", args.distinct), ("--max-mutations", args.max_mutations)):
        if value is not None:
            raise ValueError(f"--require together with {flag} is not built: the automaton conditions plain single-state designs only, and no "
                             "profile is built for it")
    if args.samples <= 0 and not profiled:
        raise ValueError("--require needs --samples N > 0")
    from rnampnn.utils.motifs import DesignAutomaton
    return dict(require=DesignAutomaton.from_motifs([m for m in args.require.split(",") if m.strip()],
                                                    [m for m in (args.avoid or "").split(",") if m.strip()], max_run=args.max_run))


def nested_option(args) -> dict:
    """The ``pairs`` and ``require`` keywords of ``predict`` from ``--pairs nested`` with ``--avoid`` / ``--max-run`` / ``--require``: one
    automaton of all of them, built (and refused) before the model is loaded; empty without ``--pairs``.  ``ValueError`` naming the flags
    with another mode or ``--profile-out``, without a motif flag, without ``--samples``, and - naming the ids - for a ``--constraints``
    table whose structures hold a pseudoknot."""
    if args.pairs is None:
        return {}
    for flag, value in (("--profile-out", args.profile_out), ("--states", args.states), ("--gc-content", args.gc_content),
                        ("--distinct", args.distinct), ("--max-mutations", args.max_mutations)):
        if value is not None:
            raise ValueError(f"--pairs nested together with {flag} is not built: the automaton conditions plain single-state designs only, and "
                             "no profile is built for it")
    if args.avoid is None and args.max_run is None and args.require is None:
        raise ValueError("--pairs nested needs --avoid, --max-run or --require: the structures of --constraints are honoured without it")
    if args.samples <= 0:
        raise ValueError("--pairs nested needs --samples N > 0")
    from rnampnn.utils.constraints import read_constraints_csv
    from rnampnn.utils.motifs import as_nested_automaton
    from rnampnn.utils.predict import check_nested_run
    split = lambda text: [m for m in (text or "").split(",") if m.strip()]
    auto = as_nested_automaton(split(args.require) if args.require is not None else None, split(args.avoid), args.max_run)
    check_nested_run(auto, None, args.samples, None, read_constraints_csv(args.constraints) if args.constraints else None)
    return dict(pairs="nested", require=auto)


def chain_option(args) -> dict:
    """The ``combine`` and ``require`` keywords of ``predict`` from ``--combine chain`` with ``--avoid`` / ``--max-run`` / ``--require``:
    one automaton of all of them, built (and refused) before the model is loaded; empty without ``--combine``.  The count comes from
    ``--gc-content`` or ``--max-mutations`` through their own options.  ``ValueError`` naming the flags with ``--profile-out``, ``--states``,
    ``--distinct``, ``--pairs`` or ``--tree global`` / ``auto``, without a motif flag, with both counts or neither, without ``--samples``,
    and - naming the ids - for a ``--constraints`` table that holds a structure."""
    if args.combine is None:
        return {}
    for flag, value in (("--profile-out", args.profile_out), ("--states", args.states), ("--distinct", args.distinct), ("--pairs", args.pairs),
                        ("--tree", None if args.tree in (None, "lds") else args.tree)):
        if value is not None:
            raise ValueError(f"--combine chain together with {flag} is not built: the chain over (position, automaton state, count) conditions "
                             "plain single-state designs on the motifs and one count, and no profile is built for it")
    if args.avoid is None and args.max_run is None and args.require is None:
        raise ValueError("--combine chain needs --avoid, --max-run or --require: a plain --gc-content or --max-mutations needs no chain")
    if (args.gc_content is None) == (args.max_mutations is None):
        raise ValueError("--combine chain needs exactly one of --gc-content and --max-mutations: two counts at once are not built")
    if args.samples <= 0:
        raise ValueError("--combine chain needs --samples N > 0")
    from rnampnn.utils.constraints import read_constraints_csv
    from rnampnn.utils.motifs import as_nested_automaton
    from rnampnn.utils.predict import check_chain_run
    split = lambda text: [m for m in (text or "").split(",") if m.strip()]
    auto = as_nested_automaton(split(args.require) if args.require is not None else None, split(args.avoid), args.max_run)
    check_chain_run(auto, None, args.samples, None, read_constraints_csv(args.constraints) if args.constraints else None)
    return dict(combine="chain", require=auto)


def profile_option(args) -> dict:
    """The ``profile_prefix`` keyword of ``predict`` from ``--profile-out``; empty without the flag.  ``ValueError`` naming the flags with
    ``--states`` or ``--distinct``."""
    if args.profile_out is None:
        return {}
    for flag, value in (("--states", args.states), ("--distinct", args.distinct)):
        if value:
            raise ValueError(f"--profile-out together with {flag} is not built: the profile is the distribution of plain, G+C, mutation-budget "
                             "and motif-avoiding single-state draws")
    return dict(profile_prefix=args.profile_out)


def table_option(args) -> dict:
    """The ``table`` keyword of ``predict`` from ``--table``; empty without the flag.  ``ValueError`` naming the flags for ``global``
    without ``--profile-out``, without a motif flag or with a mode that is not motifs alone, before the checkpoint is opened."""
    if args.table is None:
        return {}
    if args.table == "global":
        if args.profile_out is None:
            raise ValueError("--table global needs --profile-out PREFIX: it is the home of the profile's table")
        if args.require is None and args.avoid is None and args.max_run is None:
            raise ValueError("--table global needs --require, --avoid or --max-run: it is the home of the table of a profile under motifs")
        for flag, value in (("--states", args.states), ("--gc-content", args.gc_content), ("--distinct", args.distinct),
                            ("--max-mutations", args.max_mutations), ("--pairs", args.pairs), ("--combine", args.combine),
                            ("--tree", None if args.tree in (None, "lds") else args.tree)):
            if value is not None:
                raise ValueError(f"--table global together with {flag} is not built: the automaton conditions the profile on the motifs alone")
    return dict(table=args.table)


def checkpoint_family(path: str) -> str:
    """The ``model`` key of a checkpoint file; a file without one is an ``rdesign`` checkpoint.  ``weights_only=True``."""
    ck = torch.load(path, map_location="cpu", weights_only=True)
    family = ck.get("model", "rdesign") if isinstance(ck, dict) else None
    if family not in ("rnampnn", "rdesign"):
        raise ValueError(f"{path}: unknown model family {family!r}")
    return family


def run(args, log=print):
    nested = chain_option(args)                                    # --combine chain takes the motif flags into its own automaton, beside one count
    nested = nested or nested_option(args)                         # --pairs nested does the same under base pairs; a pseudoknot fails here
    require = nested or require_option(args)                       # refused with every other mode and --profile-out, before the model is loaded
    profile = profile_option(args)                                 # refused with --states / --distinct here, before the model is loaded
    avoid = {} if nested else avoid_option(args)                   # a combination that is not built fails here, before the model is loaded
    mutations = mutations_option(args)
    distinct = distinct_option(args)
    gc = gc_option(args)                                           # a bad window fails here, before the model is loaded
    tree = tree_option(args)                                       # global / auto with a mode that has no count tree fails here
    tree.update(table_option(args))                                # --table global without a profile under motifs fails here
    family = checkpoint_family(args.ckpt)
    if family == "rnampnn":
        from rnampnn.utils.predict import predict
        from rnampnn.utils.train import load_checkpoint
    else:
        from rdesign.utils.predict import predict
        from rdesign.utils.train import load_checkpoint
    extra = dict(samples=args.samples, temperature=args.temperature, seed=args.seed, designs_csv=args.designs_out, **design_options(args), **gc, **distinct,
                 **mutations, **avoid, **profile, **require, **tree)
    if args.states:
        if family != "rnampnn":
            raise ValueError("--states designs with rnampnn checkpoints only; for an rdesign checkpoint call RNAModel.design(states=...) "
                             "from Python")
        if args.samples <= 0:
            raise ValueError("--states needs --samples N > 0")
        from rnampnn.utils.constraints import read_states_csv
        extra["states"] = read_states_csv(args.states)
    model, ck = load_checkpoint(args.ckpt, device=torch.device(args.device))
    if args.xgb:
        model.load_xgb_readout(args.xgb)
    rows = predict(model, args.data, args.out, batch_size=args.batch_size, **extra)
    log(f"{len(rows)} sequences by {ck['name']} v{ck['version']} ({'tree read-out' if args.xgb else 'read-out argmax'}) written to {args.out}")
    return rows


if __name__ == "__main__":
    run(parse())
