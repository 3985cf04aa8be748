"""Directory of structures -> ``pdb_id,seq`` CSV: the role of the reference's ``rnampnn/utils/predict.py:11-29`` (a Lightning ``Trainer`` that
calls ``RNAMPNN.predict`` batch by batch) on the var-len path: ``PackedLoader`` + ``forward_packed``, so no padding is built, copied or
computed, and the letters of a batch come from one device lookup and one copy."""
from __future__ import annotations

import glob
import os
from typing import List, Optional, Tuple

import numpy as np
import torch

from ..config.glob import VOCAB
from ..model.decode import (resolve_design, check_avoid, check_budget, check_chain, check_mutations, check_profile_tree, check_table, check_tree, check_nested, check_require, design_by_mode, design_profile_from_logits, letters_packed, letters_padded,
                            sample_from_logits, score_logits)
from .constraints import batch_constraints, crossing_pairs, mutation_references, padded_references, parse_dot_bracket
from .motifs import DesignAutomaton
from .data import PackedLoader, bucket_batches, fill_nan_deterministic, read_fasta


def load_structures(path: str, max_len: int = 1 << 30):
    """``coords/<id>.npy`` (L,7,3) [+ ``seqs/<id>.fasta``] -> list of (id, coords f32, labels int64 (L,) or None) in id order.  The fasta
    is optional (the reference predicts on dummy sequences): a missing one, one of another length or one with letters outside AUCG gives
    ``None``.  Missing atoms go through ``fill_nan_deterministic``, so every structure of a usable shape gets a row."""
    items = []
    for f in sorted(glob.glob(os.path.join(path, "coords", "*.npy"))):
        rid = os.path.splitext(os.path.basename(f))[0]
        c = np.load(f, allow_pickle=False).astype(np.float32)
        if c.ndim != 3 or c.shape[1:] != (7, 3) or c.shape[0] == 0 or c.shape[0] > max_len:
            continue
        if np.isnan(c).any():
            c = fill_nan_deterministic(c, rid)
        fa, y = os.path.join(path, "seqs", rid + ".fasta"), None
        if os.path.exists(fa):
            seq = read_fasta(fa)
            if len(seq) == c.shape[0] and all(ch in VOCAB for ch in seq):
                y = np.array([VOCAB[ch] for ch in seq], dtype=np.int64)
        items.append((rid, c, y))
    return items


def state_groups(states: dict, ids: List[str], lengths: List[int]):
    """``read_states_csv`` table + the loaded structures -> [(design_id, [item index per state, file order], [weight per state])] sorted by
    ``design_id``; a structure the table does not list is a one-state design named after itself.  ``ValueError`` naming the id or the design
    for a listed structure that is not there, a ``design_id`` that is also an unlisted structure, and states that differ in length."""
    index = {rid: i for i, rid in enumerate(ids)}
    groups, listed = [], set()
    for did, rows in states.items():
        for rid, _ in rows:
            if rid not in index:
                raise ValueError(f"states: design {did!r} lists pdb_id {rid!r}, which is not among the structures")
        idx = [index[rid] for rid, _ in rows]
        if len({lengths[i] for i in idx}) > 1:
            raise ValueError(f"states: the states of design {did!r} differ in length: " + ", ".join(f"{ids[i]} = {lengths[i]}" for i in idx))
        listed.update(idx)
        groups.append((did, idx, [float(w) for _, w in rows]))
    for i, rid in enumerate(ids):
        if i not in listed:
            if rid in states:
                raise ValueError(f"states: design_id {rid!r} is also the id of a structure that no design lists")
            groups.append((rid, [i], [1.0]))
    return sorted(groups, key=lambda g: g[0])


def group_batches(groups, lengths: List[int], batch_size: int, max_rows: int) -> List[List[int]]:
    """``bucket_batches`` over whole groups: groups sorted by length are cut greedily into batches of at most ``batch_size`` rows and
    ``max_rows`` padded rows; a group larger than either gets a batch of its own.  -> lists of group indices."""
    order = sorted(range(len(groups)), key=lambda g: (lengths[groups[g][1][0]], g))
    batches, cur, rows = [], [], 0
    for g in order:
        k, n = len(groups[g][1]), lengths[groups[g][1][0]]          # ascending, so n is the longest of cur + [g]
        if cur and (rows + k > batch_size or (rows + k) * n > max_rows):
            batches.append(cur)
            cur, rows = [], 0
        cur.append(g)
        rows += k
    if cur:
        batches.append(cur)
    return batches


def draw_batch(logits, cu, max_len: int, samples: int, temperature: float, seed: int, cons=None, mode: str = "plain", **own):
    """``samples`` draws per row of one packed batch -> (draws int8 (S,B,T), seq_nll (S,B) or None, infeasible (B,) or None, *the further
    outputs of the mode's entry): from the design entry of ``mode`` (``design_by_mode``, ``own``: that mode's arguments) under constraints
    or in any mode but "plain" (they score their own draws), else free draws from ``rnampnn_sample``."""
    if cons is not None or mode != "plain":
        return design_by_mode(mode, logits, cu_seqlens=cu, max_len=max_len, n_samples=samples, temperature=temperature, seed=seed,
                              constraints=cons, **own)
    # rnampnn_sample takes the padded layout: scatter the packed logits once (row cu[b] + t -> (b, t)); the mask comes from cu
    t = torch.arange(max_len, device=logits.device)
    mask = (t[None, :] < (cu[1:] - cu[:-1])[:, None]).to(torch.float32)
    rows_of = (cu[:-1].to(torch.int64)[:, None] + t[None, :]).clamp_(max=int(logits.shape[0]) - 1)
    padded = torch.where(mask[..., None] != 0, logits[rows_of], torch.zeros((), dtype=torch.float32, device=logits.device))
    return sample_from_logits(padded, mask, temperature, samples, seed), None, None


def padded_labels(items, idx, max_len: int):
    """The fasta sequences of a batch -> (labels int32 (B, max_len), zero where there is none, or None when no row has one; have [B])."""
    have = [items[i][2] is not None for i in idx]
    if not any(have):
        return None, have
    lab = torch.zeros(len(idx), max_len, dtype=torch.int32)
    for r, i in enumerate(idx):
        if have[r]:
            lab[r, :len(items[i][2])] = torch.from_numpy(items[i][2]).to(torch.int32)
    return lab, have


def write_csv(path: str, header: str, rows) -> None:
    """``header`` and one line per row; a row is a sequence of fields that are already formatted (or ints)."""
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write(header + "\n")
        for row in rows:
            f.write(",".join(str(v) for v in row) + "\n")


def design_columns(mode: str, extras=(), lens=(), count=None):
    """The last columns that ``designs_csv`` gains in a design mode (``design_mode``) -> (their header, cells, filled): ``cells(s, r)``
    the fields of sample s of row r, ``filled`` [B] the slots of a row that hold a sequence, or None for all of them.  ``extras``: the
    two outputs of the mode's entry past (seqs, seq_nll, infeasible), ``lens`` the rows' lengths; without them only the header counts.
    ``count``: what the "chain" mode counts, "gc_content" or "mutations" (it names that mode's last two columns)."""
    if mode == "chain":                                             # six outputs: hits, accepted and count per sample, both misses and log_z per row
        hits, found, cnt, miss, cmiss, _ = (t.cpu().tolist() for t in extras) if extras else (None,) * 6
        tail = ",gc_count,gc_miss" if count == "gc_content" else ",mutations,mut_miss"
        return ",motif_hits,required_found,require_miss" + tail, lambda s, r: (hits[s][r], found[s][r], miss[r], cnt[s][r], cmiss[r]), None
    if mode == "nested":                                            # four outputs: hits and accepted per sample, dfa_miss and nest_miss per row
        hits, found, miss, nest = (t.cpu().tolist() for t in extras) if extras else (None, None, None, None)
        return ",motif_hits,required_found,require_miss,nest_miss", lambda s, r: (hits[s][r], found[s][r], miss[r], nest[r]), None
    if mode == "require":                                           # three outputs: hits and accepted per sample, dfa_miss per row
        hits, found, miss = (t.cpu().tolist() for t in extras) if extras else (None, None, None)
        return ",motif_hits,required_found,require_miss", lambda s, r: (hits[s][r], found[s][r], miss[r]), None
    per_sample, per_row = (t.cpu().tolist() for t in extras) if extras else (None, None)
    if mode == "gc_content":
        return ",gc,gc_miss", lambda s, r: (f"{per_sample[s][r] / lens[r]:.6f}", per_row[r]), None
    if mode == "mutations":
        return ",mutations,mut_miss", lambda s, r: (per_sample[s][r], per_row[r]), None
    if mode == "avoid":
        return ",motif_hits,avoid_miss", lambda s, r: (per_sample[s][r], per_row[r]), None
    if mode == "distinct":
        return ",logp", lambda s, r: (f"{per_sample[s][r]:.6f}",), per_row
    return "", lambda s, r: (), None


def check_profile(profile_prefix, states=None, distinct=None) -> None:
    """``predict(..., profile_prefix=...)``: ``ValueError`` with ``states`` or ``distinct`` - no profile is built for multi-state or distinct
    designs; touches no device."""
    if profile_prefix and (states is not None or distinct is not None):
        raise ValueError("a design profile together with states or distinct is not built: the profile is the distribution of plain, G+C, "
                         "mutation-budget and motif-avoiding single-state draws")


def refuse_structures(what: str, constraints) -> None:
    """``ValueError`` naming the first ids of a constraints table whose ``structure`` is not empty: ``what`` is not built with base pairs."""
    paired = sorted(rid for rid, (_, structure) in (constraints or {}).items() if structure)
    if paired:
        raise ValueError(f"{what} together with base pairs is not built (an exact draw would carry every open pair in the automaton's "
                         f"state): drop `structure` from the constraints of {paired[:3]}{' ...' if len(paired) > 3 else ''}")


def check_require_run(require, avoid, samples: int, profile_prefix, constraints, table: str = "lds") -> object:
    """``predict(..., require=...)`` -> the ``DesignAutomaton`` that holds ``require`` and ``avoid``, or None without ``require``.
    ``ValueError`` without samples, with a profile (none is built for this mode in LDS: ``table="global"`` opts in to
    ``rnampnn_design_dfa_profile``, with or without samples) and with a structure in ``constraints``; touches no device."""
    auto = check_require(require, avoid)
    if auto is None:
        return None
    if profile_prefix and table != "global":
        raise ValueError("a design profile together with require is not built: the profile entries know forbidden motifs only")
    if samples <= 0 and not (profile_prefix and table == "global"):
        raise ValueError("required motifs need samples > 0")
    refuse_structures("require", constraints)
    return auto


def check_chain_run(require, avoid, samples: int, profile_prefix, constraints) -> object:
    """``predict(..., combine="chain")`` -> the ``DesignAutomaton`` of ``require`` and / or ``avoid`` (``check_chain``).  ``ValueError``
    without samples, with a profile (none is built for this mode) and with a structure in ``constraints``; touches no device."""
    auto = check_chain(None, require, avoid)
    if profile_prefix:
        raise ValueError("a design profile together with combine='chain' is not built: the profile entries know a count or forbidden motifs, "
                         "not both")
    if samples <= 0:
        raise ValueError("motifs under a count window need samples > 0")
    refuse_structures("combine='chain'", constraints)
    return auto


def check_nested_run(require, avoid, samples: int, profile_prefix, constraints) -> object:
    """``predict(..., pairs="nested")`` -> the ``DesignAutomaton`` of ``require`` and / or ``avoid`` (``check_nested``).  ``ValueError``
    without samples, with a profile (none is built for this mode) and, naming the ids, for a constraints table whose structures hold a
    pseudoknot; touches no device."""
    auto = check_nested(require, avoid)
    if profile_prefix:
        raise ValueError("a design profile together with pairs='nested' is not built: the profile entries know no automaton under base pairs")
    if samples <= 0:
        raise ValueError("motifs under a nested structure need samples > 0")
    knotted = []
    for rid, (_, structure) in sorted((constraints or {}).items()):
        try:
            if structure and crossing_pairs(parse_dot_bracket(structure)):
                knotted.append(rid)
        except ValueError as exc:
            raise ValueError(f"constraints for {rid}: {exc}") from None
    if knotted:
        raise ValueError(f"pairs='nested': the structure of {knotted[:3]}{' ...' if len(knotted) > 3 else ''} holds a pseudoknot (two of its "
                         "pairs cross); the exact draw under motifs walks a nested structure: drop the crossing pairs")
    return auto


def check_avoid_run(avoid, samples: int, profile_prefix, constraints) -> object:
    """``predict(..., avoid=...)`` without ``require`` -> the ``MotifAutomaton``, or None without ``avoid``.  ``ValueError`` without
    samples or a profile and with a structure in ``constraints``; touches no device."""
    auto = check_avoid(avoid)
    if auto is None:
        return None
    if samples <= 0 and not profile_prefix:
        raise ValueError("forbidden motifs need samples > 0")
    refuse_structures("avoid", constraints)
    return auto


def resolve_run(samples: int, profile_prefix, constraints, states=None, **given):
    """``resolve_design`` as both command-line ``predict`` call it, before the first forward pass -> (mode, avoid, require): the checks
    in their ``*_run`` forms, which know ``samples``, the profile and the constraints TABLE; ``given``: gc_content, distinct, mutations
    (min, max, references), avoid, require, pairs, combine, tree, and ``table`` ("lds", the default: nothing differs; "global": the
    profile of ``require`` and / or ``avoid`` comes from ``rnampnn_design_dfa_profile`` - ``check_table``, which needs a profile and a
    mode of motifs alone)."""
    table = given.pop("table", "lds")

    def run(tree, mode):
        check_tree(tree, mode) if samples > 0 or not profile_prefix else check_profile_tree(tree, mode)
        check_profile(profile_prefix, states, given.get("distinct"))
        if table != "lds":
            check_table(table, None, given.get("gc_content"), given.get("mutations"), given.get("avoid"), given.get("require"), None, tree)
            if not profile_prefix or mode not in ("require", "avoid"):
                raise ValueError(f"table={table!r} is the home of the table of a design profile under avoid and / or require: it needs "
                                 "profile_prefix and none of states, distinct, pairs and combine")
        return [lambda r, a, f=f: f(r, a, samples, profile_prefix, constraints) for f in (check_chain_run, check_nested_run)] + [
            lambda r, a: check_require_run(r, a, samples, profile_prefix, constraints, table),
            lambda a: check_avoid_run(a, samples, profile_prefix, constraints)]
    mode, mutations, avoid, require = resolve_design(states=states, run=run, **given)
    if mutations is not None:
        check_budget(mutations[0], mutations[1])
        if samples <= 0 and not profile_prefix:
            raise ValueError("a mutation budget needs samples > 0")
    return mode, avoid, require


def profile_automaton(avoid, require, table: str = "lds"):
    """The automaton of a run's profiles, once per run, from ``resolve_run``'s result: ``require``, else ``avoid`` (a ``DesignAutomaton`` with ``table="global"``)."""
    return require if require is not None else DesignAutomaton.from_avoid(avoid) if avoid is not None and table == "global" else avoid


def profile_batch(store: dict, idx, lens, logits, cu, max_len: int, temperature: float, cons, gc_content, mutations, tree: str, mode: str,
                  auto) -> None:
    """The design profile of one packed batch (``design_profile_from_logits`` on ``resolve_run``'s ``mode`` and ``profile_automaton``'s ``auto``; ``mutations`` as ``design`` takes it) into ``store``:
    item index -> (marginals [n][4], log_mass, entropy, infeasible, miss).  One launch, one copy per output."""
    prof = design_profile_from_logits(logits, cu_seqlens=cu, max_len=max_len, temperature=temperature, constraints=cons, gc_content=gc_content,
                                      tree=tree, resolved=(mode, check_mutations(mutations), auto))
    marg, mass, ent = prof.marginals.cpu().tolist(), prof.log_mass.cpu().tolist(), prof.entropy.cpu().tolist()
    bad, miss = prof.infeasible.cpu().tolist(), prof.miss.cpu().tolist()
    for r, i in enumerate(idx):
        store[i] = (marg[r][:lens[r]], mass[r], ent[r], bad[r], miss[r])


def write_profile(prefix: str, ids, store: dict) -> None:
    """``PREFIX.positions.csv`` (``pdb_id,position,pA,pU,pC,pG``, one row per nucleotide, 1-based) and ``PREFIX.rnas.csv``
    (``pdb_id,length,log_mass,entropy,infeasible,miss``) in id order; floats as ``repr`` writes them, so they read back exactly."""
    write_csv(prefix + ".positions.csv", "pdb_id,position,pA,pU,pC,pG",
              [(rid, t + 1) + tuple(repr(float(v)) for v in row) for i, rid in enumerate(ids) for t, row in enumerate(store[i][0])])
    write_csv(prefix + ".rnas.csv", "pdb_id,length,log_mass,entropy,infeasible,miss",
              [(rid, len(store[i][0]), repr(float(store[i][1])), repr(float(store[i][2])), store[i][3], store[i][4]) for i, rid in enumerate(ids)])


@torch.no_grad()
def predict(model, data_path: str, out_csv: str, batch_size: int = 32, max_rows: int = 32768, samples: int = 0, temperature: float = 0.1,
            seed: int = 0, designs_csv: Optional[str] = None, constraints: Optional[dict] = None, bias=None, omit: str = "",
            wobble: bool = True, states: Optional[dict] = None, gc_content=None, distinct=None, mutations=None,
            avoid=None, profile_prefix: Optional[str] = None, require=None, pairs=None, tree: str = "lds", combine=None, table: str = "lds") -> List[Tuple[str, str]]:
    """Design a sequence for every structure under ``data_path`` in length-bucketed var-len batches (``forward_packed``): the tree
    read-out on the packed embedding when one is attached, else the read-out's argmax (``rnampnn_score``'s ``pred``); write ``out_csv``
    with one ``pdb_id,seq`` row per structure in id order.  -> the rows.  ``samples > 0``: also draw that many sequences per structure
    at ``temperature`` (``rnampnn_sample``), score them against the same logits and write ``designs_csv`` with the columns
    ``pdb_id,sample,seq,nll_per_nt,recovery`` (``recovery`` = fraction equal to the fasta's sequence, empty without one).
    ``constraints`` ({pdb_id: (pattern, structure)}, ``read_constraints_csv``; ids not in it are unconstrained), ``bias`` (4 per-class
    floats), ``omit`` (letters never drawn) or ``wobble=False``: the draws come from ``rnampnn_design`` on the packed logits instead (no
    scatter to the padded layout) and ``designs_csv`` gains a last column ``infeasible``.
    ``states`` (``read_states_csv``: {design_id: [(pdb_id, weight)]}): multi-state design - the batches are formed from whole designs with
    their states as consecutive rows, the draws come from ``rnampnn_design_tied`` and ``designs_csv`` has one row per (design, sample):
    ``design_id,sample,seq,infeasible,states,nll_per_nt,recovery``, the last three ``;``-joined per state.
    ``gc_content`` (lo, hi): the draws - constrained or free - come from ``rnampnn_design_gc``, conditioned exactly on the G+C fraction of
    every structure lying in that window; ``designs_csv`` gains the last columns ``gc`` (the fraction of the draw) and ``gc_miss`` (0, or
    how many nucleotides the nearest reachable count lies outside the window).  Not built together with ``states``.
    ``distinct`` ("sample" / "best"): the draws - constrained or free - come from ``rnampnn_design_distinct`` and are pairwise different per
    structure (a sample without replacement / the most probable sequences in descending order); ``designs_csv`` gains a last column
    ``logp`` and holds no row for a slot the structure's admitted sequences do not fill.  Not built together with ``states`` or
    ``gc_content``.
    ``mutations`` (min, max, references): a mutation budget - the draws, constrained or free, come from ``rnampnn_design_count`` and differ
    from the structure's reference sequence at between min and max positions, drawn exactly from the model's distribution conditioned on
    that.  ``references`` is {pdb_id: sequence} (``read_reference_fasta``) or None for the structure's own ``seqs/<id>.fasta``; a
    structure without a reference is a ``ValueError`` naming its id.  ``designs_csv`` gains the last columns ``mutations`` (the Hamming
    distance of the draw to the reference) and ``mut_miss`` (0, or by how many mutations the structure and the fixed positions alone
    exceed the budget).  Not built together with ``states``, ``gc_content`` or ``distinct``.
    ``avoid`` (a ``MotifAutomaton`` or motif strings): forbidden motifs - the draws come from ``rnampnn_design_avoid`` and contain none of
    them, drawn exactly from the model's distribution conditioned on that and on the fixed positions, ``omit`` and ``bias``.
    ``designs_csv`` gains the last columns ``motif_hits`` (positions of the draw at which a motif ends: 0 unless ``avoid_miss``) and
    ``avoid_miss`` (1 for a structure whose fixed positions spell a motif).  Not built together with the other modes; a constraints
    table with a structure column that is not empty is a ``ValueError`` before the first forward pass.
    ``require`` (a ``DesignAutomaton`` or motif strings): required motifs - the draws come from ``rnampnn_design_dfa`` and contain EVERY one
    of them somewhere and none of ``avoid``, which it absorbs.  ``designs_csv`` gains the last columns ``motif_hits``, ``required_found``
    (1 when the draw holds every required motif) and ``require_miss`` (1 for a structure that cannot hold them: too short, or its fixed
    positions rule one out).  Not built together with the other modes, a profile or a structure in ``constraints``.
    ``pairs="nested"``: ``avoid`` and / or ``require`` UNDER the structures of ``constraints`` - the draws come from
    ``rnampnn_design_nested``; ``designs_csv`` gains the last columns ``motif_hits``, ``required_found``, ``require_miss`` and
    ``nest_miss``.  A structure with a pseudoknot is a ``ValueError`` naming its ids before the first forward pass; not built together with
    the other modes or a profile.
    ``profile_prefix``: also write the design profile of every structure - the exact distribution the draws of the chosen mode come from
    under ``temperature`` and the constraints (``design_profile_from_logits``) - to ``PREFIX.positions.csv`` and ``PREFIX.rnas.csv``
    (``write_profile``), with or without ``samples``.  Not built together with ``states`` or ``distinct``.
    ``tree`` ("lds", the default: everything above, unchanged; "global"; "auto"): where the count tree of ``gc_content`` and ``mutations``
    and of their profiles lives (``check_tree``); in global memory structures longer than the 1,017 nt a G+C window fits in LDS are
    designed.  Anything but "lds" with another mode is a ``ValueError`` before the first forward pass.
    ``combine="chain"`` (``None`` is everything above, unchanged): ``avoid`` and / or ``require`` TOGETHER with ``gc_content`` or
    ``mutations`` - the draws come from ``rnampnn_design_dfa_count`` and hold both conditions exactly; ``designs_csv`` gains the last
    columns ``motif_hits``, ``required_found``, ``require_miss`` and then ``gc_count``, ``gc_miss`` or ``mutations``, ``mut_miss``.  Not
    built together with ``states``, ``distinct``, ``pairs``, a profile, a ``tree`` other than "lds" or a ``structure`` in ``constraints``.
    ``table`` ("lds", the default: everything above, unchanged; "global"): with ``profile_prefix`` and ``require`` and / or ``avoid``, the
    profile comes from ``rnampnn_design_dfa_profile`` - the distribution ``rnampnn_design_dfa`` draws from, on automata of up to 256
    states, with or without ``samples``; the files keep their columns and ``miss`` holds ``dfa_miss``.  The draws stay
    ``rnampnn_design_dfa``'s for ``require`` and ``rnampnn_design_avoid``'s for ``avoid`` alone.  Without a profile, or with another mode,
    it is a ``ValueError`` before the first forward pass."""
    mode, avoid, require = resolve_run(samples, profile_prefix, constraints, states, gc_content=gc_content, distinct=distinct, mutations=mutations,
                                       avoid=avoid, require=require, pairs=pairs, combine=combine, tree=tree, table=table)
    count = "gc_content" if gc_content is not None else "mutations"     # (what the chain counts: it names its columns)
    profiled = profile_automaton(avoid, require, table)
    model.eval()
    device = model._device()
    items = load_structures(data_path, max_len=int(model.hparams["padding_len"]))
    if not items:
        raise ValueError(f"no usable structure under {data_path} (coords/<id>.npy (L,7,3))")
    if samples > 0 and not designs_csv:
        designs_csv = os.path.splitext(out_csv)[0] + "_designs.csv"
    ids, lengths = [it[0] for it in items], [int(it[1].shape[0]) for it in items]
    refs = None if mutations is None else mutation_references(mutations[2], ids, lengths, [it[2] for it in items])
    trees = getattr(model, "xgb_readout", None)
    constrained = constraints is not None or bias is not None or bool(omit) or not wobble
    seqs, designs, profiles = {}, {}, {}
    groups = batch_groups = None
    if states is not None:
        if samples <= 0:
            raise ValueError("multi-state design needs samples > 0")
        groups = state_groups(states, ids, lengths)
        batch_groups = group_batches(groups, lengths, batch_size, max_rows)
        batches = [[i for g in gs for i in groups[g][1]] for gs in batch_groups]
    else:
        batches = bucket_batches(lengths, batch_size, max_rows, seed=0)
    for bi, (coords, cu, max_len, idx) in enumerate(PackedLoader(items, batches, device=device)):
        lens = [lengths[i] for i in idx]
        if trees is not None:
            logits, emb = model.forward_packed(coords, cu, max_len, want_embedding=True)
            names = letters_packed(trees.predict(emb), lens)
        else:
            logits = model.forward_packed(coords, cu, max_len)
            names = letters_padded(score_logits(logits, cu_seqlens=cu, want=("pred",), max_len=max_len)["pred"])
        seqs.update(zip(idx, names))
        if samples <= 0 and not profile_prefix:
            continue
        gs = None if groups is None else batch_groups[bi]
        cons = None
        if constrained:
            cons = batch_constraints(constraints, [ids[i] for i in idx], lens, max_len, bias=bias, wobble=wobble, omit=omit).to_device(device)
        if profile_prefix:
            profile_batch(profiles, idx, lens, logits, cu, max_len, temperature, cons, gc_content,
                          None if mutations is None else (padded_references(refs, idx, max_len), mutations[0], mutations[1]), tree, mode,
                          profiled)
        if samples <= 0:
            continue
        draws, dnll, bad, *extras = draw_batch(
            logits, cu, max_len, samples, temperature, seed + bi, cons, mode, gc_content=gc_content, distinct=distinct, avoid=avoid, require=require,
            mutations=None if mutations is None else (padded_references(refs, idx, max_len), (mutations[0], mutations[1])),
            states=None if gs is None else [len(groups[g][1]) for g in gs],
            state_weights=None if gs is None else [w for g in gs for w in groups[g][2]], tree=tree)
        if not constrained and gs is None:
            bad = None                                              # the column belongs to the constrained forms
        _, cells, filled = design_columns(mode, extras, lens, count)
        bad = None if bad is None else bad.cpu().tolist()
        lab, have = padded_labels(items, idx, max_len)
        want = (("seq_nll",) if dnll is None else ()) + (("seq_match",) if lab is not None else ())      # rnampnn_design scores its own draws
        sc = score_logits(logits, cu_seqlens=cu, labels=lab, seqs=draws, want=want) if want else {}
        nll = (sc["seq_nll"] if dnll is None else dnll).cpu().tolist()
        match = sc["seq_match"].cpu().tolist() if lab is not None else None
        for s in range(samples):
            text = letters_padded(draws[s])
            recs = [f"{match[s][r] / lens[r]:.6f}" if have[r] else "" for r in range(len(idx))]
            if gs is None:
                for r, i in enumerate(idx):
                    if filled is not None and s >= filled[r]:
                        continue                                    # fewer admitted sequences than samples: the slot is empty
                    designs.setdefault(i, []).append((s, text[r], f"{nll[s][r] / lens[r]:.6f}", recs[r]) + (() if bad is None else (bad[r],))
                                                     + cells(s, r))
                continue
            r = 0
            for g in gs:                                            # one row per (design, sample); the states are consecutive rows
                rows = range(r, r + len(groups[g][1]))
                designs.setdefault(g, []).append((s, text[r], bad[r], ";".join(ids[idx[k]] for k in rows),
                                                  ";".join(f"{nll[s][k] / lens[k]:.6f}" for k in rows), ";".join(recs[k] for k in rows)))
                r += len(rows)
    rows = [(rid, seqs[i]) for i, rid in enumerate(ids)]
    write_csv(out_csv, "pdb_id,seq", rows)
    if profile_prefix:
        write_profile(profile_prefix, ids, profiles)
    if groups is not None:
        write_csv(designs_csv, "design_id,sample,seq,infeasible,states,nll_per_nt,recovery",
                  [(group[0],) + row for g, group in enumerate(groups) for row in designs[g]])
    elif samples > 0:
        write_csv(designs_csv, "pdb_id,sample,seq,nll_per_nt,recovery" + (",infeasible" if constrained else "") + design_columns(mode, count=count)[0],
                  [(rid,) + row for i, rid in enumerate(ids) for row in designs[i]])
    return rows
