"""MI355X-native mirror of the reference's sibling package ``rdesign``: the ``RNAModel`` forward
(k-NN graph, RBF / orientation / dihedral features, ``MPNNLayer`` stack, read-out) behind the reference's module names, computed by
``librnampnn_hip.so`` (C ABI: ``include/rdesign_hip.h``).  Parity: pinned to the reference's own modules in eval mode by
``tests/golden/rdesign_*.npz`` - see ``oracle/rdesign_oracle.py``.  ``rdesign.utils`` holds the host pipeline around it: the reference's
collate and a 6-atom loader (``data``), the epoch trainer and checkpoints (``train``) and the directory -> CSV driver (``predict``)."""
