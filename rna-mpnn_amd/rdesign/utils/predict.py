"""Directory of structures -> ``pdb_id,seq`` CSV: the role of the reference's ``main.py:17-31`` + ``rdesign/utils/predict.py:10-30``."""
from __future__ import annotations

import os
from typing import List, Optional, Tuple

from rnampnn.model.decode import design_by_mode, letters_padded, score_logits
from rnampnn.utils.constraints import batch_constraints, mutation_references, padded_references
from rnampnn.utils.data import bucket_batches
from rnampnn.utils.predict import design_columns, profile_automaton, profile_batch, resolve_run, write_csv, write_profile

from .data import load_rna_dir, padded_loader


def predict(model, data_path: str, out_csv: str, batch_size: int = 32, max_rows: int = 32768, samples: int = 0, temperature: float = 0.1,
            seed: int = 0, designs_csv: Optional[str] = None, constraints: Optional[dict] = None, bias=None, omit: str = "",
            wobble: bool = True, gc_content=None, distinct=None, mutations=None, avoid=None,
            profile_prefix: Optional[str] = None, require=None, pairs=None, tree: str = "lds", combine=None,
            table: str = "lds") -> List[Tuple[str, str]]:
    """Read ``data_path`` (``coords/<id>.npy`` + ``seqs/<id>.fasta``), design a sequence for every structure in length-bucketed batches
    (``RNAModel.predict_sequences``: the tree read-out when one is attached, else the read-out's argmax) and write ``out_csv`` with one
    ``pdb_id,seq`` row per input in id order.  -> the rows.  ``samples > 0``: also draw that many sequences per structure at
    ``temperature`` from the packed read-out logits with ``rnampnn_design`` - under ``constraints`` ({pdb_id: (pattern, structure)}; ids
    not in it are unconstrained), ``bias`` (4 per-class floats), ``omit`` (letters never drawn) and ``wobble`` - and write ``designs_csv``
    with the columns ``pdb_id,sample,seq,nll_per_nt,recovery,infeasible``.  ``gc_content`` (lo, hi): the draws come from
    ``rnampnn_design_gc``, conditioned exactly on the G+C fraction of every structure lying in that window, and ``designs_csv`` gains the
    last columns ``gc`` (the fraction of the draw) and ``gc_miss``.  ``distinct`` ("sample" / "best"): the draws come from
    ``rnampnn_design_distinct`` and are pairwise different per structure; ``designs_csv`` gains a last column ``logp`` and holds no row for
    a slot the structure's admitted sequences do not fill.  Not built together with ``gc_content``.  ``mutations`` (min, max, references):
    a mutation budget - the draws come from ``rnampnn_design_count`` and differ from the reference sequence of the structure
    (``references[pdb_id]``, or with None its own fasta sequence) at between min and max positions; ``designs_csv`` gains the last columns
    ``mutations`` and ``mut_miss``.  Not built together with ``gc_content`` or ``distinct``.  ``avoid`` (a ``MotifAutomaton`` or motif
    strings): the draws come from ``rnampnn_design_avoid`` and contain none of the motifs; ``designs_csv`` gains the last columns
    ``motif_hits`` and ``avoid_miss``.  Not built together with the other modes or with a structure in ``constraints``.
    ``require`` (a ``DesignAutomaton`` or motif strings): the draws come from ``rnampnn_design_dfa`` and contain every one of the motifs
    and none of ``avoid``, which it absorbs; ``designs_csv`` gains the last columns ``motif_hits``, ``required_found`` and
    ``require_miss``.  Not built together with the other modes, a profile or a structure in ``constraints``.
    ``pairs="nested"``: ``avoid`` and / or ``require`` UNDER the structures of ``constraints`` - the draws come from
    ``rnampnn_design_nested``; ``designs_csv`` gains the last columns ``motif_hits``, ``required_found``, ``require_miss`` and
    ``nest_miss``.  A structure with a pseudoknot is a ``ValueError`` naming its ids before the first forward pass.
    ``profile_prefix``: also write the design profile of every structure (``design_profile_from_logits``: the exact distribution the
    draws of the chosen mode come from) to ``PREFIX.positions.csv`` and ``PREFIX.rnas.csv``, with or without ``samples``.  Not built
    together with ``distinct``.  ``tree`` ("lds", the default; "global"; "auto"): where the count tree of ``gc_content`` and ``mutations``
    and of their profiles lives (``check_tree``); anything but "lds" with another mode is a ``ValueError`` before the first forward pass.
    ``combine="chain"``: ``avoid`` and / or ``require`` TOGETHER with ``gc_content`` or ``mutations`` (``rnampnn_design_dfa_count``), as in
    ``rnampnn.utils.predict.predict``: the same columns and the same refusals.  ``table="global"``: the profile of ``require`` and / or
    ``avoid`` from ``rnampnn_design_dfa_profile``, as there."""
    mode, avoid, require = resolve_run(samples, profile_prefix, constraints, gc_content=gc_content, distinct=distinct, mutations=mutations,
                                       avoid=avoid, require=require, pairs=pairs, combine=combine, tree=tree, table=table)
    count = "gc_content" if gc_content is not None else "mutations"     # (what the chain counts: it names its columns)
    model.eval()
    items = load_rna_dir(data_path)
    if not items:
        raise ValueError(f"no usable structure under {data_path} (coords/<id>.npy (L,7,3) + seqs/<id>.fasta)")
    if samples > 0 and not designs_csv:
        designs_csv = os.path.splitext(out_csv)[0] + "_designs.csv"
    refs = None if mutations is None else mutation_references(mutations[2], [it[0] for it in items], [it[1].shape[0] for it in items],
                                                              [it[2] for it in items])
    batches = bucket_batches([c.shape[0] for _, c, _ in items], batch_size, max_rows, seed=0)
    device = model._device()
    profiled = profile_automaton(avoid, require, table)
    seqs, designs, profiles = {}, {}, {}
    for bi, (S, X, mask, lengths, idx) in enumerate(padded_loader(items, batches, device=device)):
        for i, s in zip(idx, model.predict_sequences(X, mask, lengths)):
            seqs[i] = s
        if samples > 0 or profile_prefix:
            lens = [int(v) for v in lengths]
            logits, cu, T = model._packed_logits(X, mask, lengths)
            cons = batch_constraints(constraints, [items[i][0] for i in idx], lens, T, bias=bias, wobble=wobble, omit=omit)
        if profile_prefix:
            profile_batch(profiles, idx, lens, logits, cu, T, temperature, cons.to_device(device), gc_content,
                          None if mutations is None else (padded_references(refs, idx, T), mutations[0], mutations[1]), tree, mode, profiled)
        if samples > 0:
            draws, nll, bad, *extras = design_by_mode(
                mode, logits, cu_seqlens=cu, max_len=T, n_samples=samples, temperature=temperature, seed=seed + bi,
                constraints=cons.to_device(device), gc_content=gc_content, distinct=distinct, avoid=avoid, require=require,
                mutations=None if mutations is None else (padded_references(refs, idx, T), (mutations[0], mutations[1])), tree=tree)
            _, cells, filled = design_columns(mode, extras, lens, count)
            match = score_logits(logits, cu_seqlens=cu, labels=S, seqs=draws, want=("seq_match",))["seq_match"].cpu().tolist()
            nll, bad = nll.cpu().tolist(), bad.cpu().tolist()
            for s in range(samples):
                for r, (i, text) in enumerate(zip(idx, letters_padded(draws[s]))):
                    if filled is not None and s >= filled[r]:
                        continue                                    # fewer admitted sequences than samples: the slot is empty
                    designs.setdefault(i, []).append((s, text, f"{nll[s][r] / lens[r]:.6f}", f"{match[s][r] / lens[r]:.6f}", bad[r]) + cells(s, r))
    rows = [(items[i][0], seqs[i]) for i in range(len(items))]
    write_csv(out_csv, "pdb_id,seq", rows)
    if profile_prefix:
        write_profile(profile_prefix, [it[0] for it in items], profiles)
    if samples > 0:
        write_csv(designs_csv, "pdb_id,sample,seq,nll_per_nt,recovery,infeasible" + design_columns(mode, count=count)[0],
                  [(it[0],) + row for i, it in enumerate(items) for row in designs[i]])
    return rows
