#!/usr/bin/env python3
"""The forward taps and the training gradients that pass through the node side (GraphNorm statistics, node update, GraphNorm backward), as .npy
files: the byte comparison of two builds of the library (docs/experiments.md, "the node side folded").  Plain dumping - no timing, no
profiler, no retry.
usage: python tools/node_side_dump.py <outdir>          one child process per leg, each under its own `timeout`, stopping at the first that
                                                        fails; then the number of dumps, their size and one sha256 over all of them
       python tools/node_side_dump.py <outdir> <leg>    that leg, in this process
RNAMPNN_PROBE_ROOT: another checkout (with its library built) to take the package from, as in tools/design_dump.py; only API that the parent
of this tool's commit has is used.  Compare two runs with `diff -r <outdir a> <outdir b>` or by the printed sha256.
Model: the small closed-form-weight model of tests/test_round4_gpu.py::_small (3 ResMPNN layers, k = 30, padding_len = T), bf16 and f32.
Forward legs `fwd.<precision>.T<T>.<one|two>`: the batches of FORWARD below (synth_batch, first_index 11), with the per-RNA node update and with
RNAMPNN_NODE_UPDATE_TWO_LAUNCH=1; logits, h0, h_post, raw_emb and h_layer / e_layer of every layer.  Training legs `train.<precision>.T<T>`:
loss_and_grad(seed=9) with the model's dropout on the T = 64 batch and the T = 520 one (the split GraphNorm backward); loss and flat_grad."""
import hashlib
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.environ.get("RNAMPNN_PROBE_ROOT") or os.path.join(HERE, "..")
SWITCH = "RNAMPNN_NODE_UPDATE_TWO_LAUNCH"
LAYERS = 3
FORWARD = {                                               # T: lens - what the batch reaches
    24: [24, 1, 17],                                      # statistics <8,20>; two-launch update (T < 48); k_gn_coef 5-row branch
    64: [64, 20, 47, 33, 5, 58, 31, 1],                   # per-RNA update, 4 row blocks
    150: [150, 97, 1, 129, 33, 140],                      # 5 row blocks
    200: [200, 161, 1, 77],                               # <8,32>; 8 row blocks; with the switch the 8- and 5-row k_gn_coef branches
    300: [300, 257, 1, 40],                               # <8,0>; two-launch; k_gn_coef loop branch
    520: [520, 513, 1, 33],                               # <32,0>
}
TRAIN = (64, 520)                                         # 520 > GN_SPLIT_T: the split backward
LEGS = tuple(f"fwd.{p}.T{T}.{f}" for p in ("bf16", "f32") for T in FORWARD for f in ("one", "two")) + \
       tuple(f"train.{p}.T{T}" for p in ("bf16", "f32") for T in TRAIN)


def dump_leg(outdir: str, leg: str) -> None:
    kind, precision, T, form = (leg.split(".") + [""])[:4]
    T = int(T[1:])
    if form == "two":
        os.environ[SWITCH] = "1"
    else:
        os.environ.pop(SWITCH, None)
    sys.path.insert(0, os.path.join(ROOT, "rna-mpnn_amd"))
    import numpy as np
    import torch
    from rnampnn import _native
    from rnampnn.model.rnampnn import RNAMPNN
    from rnampnn.utils import synth
    assert os.path.realpath(_native.__file__).startswith(os.path.realpath(ROOT)), (_native.__file__, ROOT)
    _native.lib()
    os.makedirs(outdir, exist_ok=True)

    torch.manual_seed(5)
    model = RNAMPNN(precision=precision, num_res_neighbours=30, num_res_mpnn_layers=LAYERS, padding_len=T)
    sd = synth.closed_form_state_dict({k: tuple(v.shape) for k, v in model.state_dict().items()})
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    model = model.to("cuda:0")
    coords, mask, labels = synth.synth_batch(FORWARD[T], first_index=11)
    assert coords.shape[1] == T
    c, m = torch.from_numpy(coords), torch.from_numpy(mask)

    def save(name, t):
        np.save(os.path.join(outdir, f"{leg}.{name}.npy"), t.detach().cpu().numpy())

    if kind == "fwd":
        model.eval()
        save("logits", model(c, m))
        for layer in range(1, LAYERS + 1):
            taps = model.forward_taps(c, m, ["h0", "h_layer", "e_layer", "h_post", "raw_emb"], tap_layer=layer)
            save(f"h_layer{layer}", taps["h_layer"])
            save(f"e_layer{layer}", taps["e_layer"])
            if layer == 1:
                for name in ("h0", "h_post", "raw_emb"):
                    save(name, taps[name])
    elif kind == "train":
        model.train()
        loss = model.loss_and_grad(torch.from_numpy(labels), c, m, seed=9)
        save("loss", loss)
        save("flat_grad", model.flat_grad)
    else:
        raise SystemExit(f"unknown leg {leg!r}: choose from {LEGS}")
    torch.cuda.synchronize()
    print(f"{leg}: dumped from {os.path.realpath(_native.LIB_PATH)}")


def main() -> int:
    if len(sys.argv) < 2:
        raise SystemExit(__doc__)
    outdir = os.path.abspath(sys.argv[1])
    if len(sys.argv) > 2:
        dump_leg(outdir, sys.argv[2])
        return 0
    for leg in LEGS:
        rc = subprocess.run(["timeout", "-k", "10", "120", sys.executable, os.path.abspath(__file__), outdir, leg]).returncode
        if rc != 0:
            print(f"{leg}: exit status {rc}; nothing further is started")
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
