"""Error measure of an h / e tap against a reference, and the valid-row selection both need (numpy / torch, no GPU).

A tap is looked at as a matrix of valid rows x 128 channels: for ``e`` the edges with ``edge_index != -1`` of valid residues, for ``h``
the valid residues.  ``G`` is the result under test, ``R`` the reference:

    ch[c]  = rms_rows(G - R)[c] / max(rms_rows(R)[c], 0.25 * median_c rms_rows(R))      one figure per channel
    row[i] = rms_ch(G - R)[i]   / max(rms_ch(R)[i],   0.25 * median_i rms_ch(R))        one figure per row
    absmax = max |G - R|

A channel routed to the wrong place shows in ``ch`` (the logits and even the h taps dilute it: mean over k, GraphNorm); a wrong row - a
wrong neighbour gathered, a block written to the wrong place, the tail of a tile - shows in ``row``.  The floors at a quarter of the median
keep a nearly silent channel or row from turning rounding noise into a large ratio.  A per-channel rms over a handful of rows is noise, so
``max ch`` is only meaningful (``TapError.ch_ok``) from ``MIN_ROWS_FOR_CH`` valid rows on.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

MIN_ROWS_FOR_CH = 256
FLOOR = 0.25


@dataclass
class TapError:
    rows: int
    max_ch: float
    med_ch: float
    max_row: float
    med_row: float
    absmax: float
    worst_ch: int
    worst_row: int
    max_row_rms: float          # largest rms over the channels of (G - R) of one row, in units of the tap

    @property
    def ch_ok(self) -> bool:
        return self.rows >= MIN_ROWS_FOR_CH

    def __str__(self) -> str:
        return (f"rows {self.rows:6d}  ch max {self.max_ch:.3e} (c {self.worst_ch:3d}) med {self.med_ch:.3e}  "
                f"row max {self.max_row:.3e} (i {self.worst_row}) med {self.med_row:.3e}  absmax {self.absmax:.3e}")


def _np(x) -> np.ndarray:
    if hasattr(x, "detach"):
        x = x.detach().cpu().numpy()
    return np.asarray(x)


def valid_rows(tap, mask, edge_index=None) -> np.ndarray:
    """The valid rows of a padded tap as a float64 (rows, D) matrix: ``h`` (B,T,D) with ``mask`` (B,T); ``e`` (B,T,k,D) with
    ``edge_index`` (B,T,k) as well (slots holding -1 and every slot of a padded residue are left out)."""
    tap, ok = _np(tap).astype(np.float64), _np(mask) > 0
    if edge_index is not None:
        ok = ok[..., None] & (_np(edge_index) != -1)
    assert tap.shape[:-1] == ok.shape, (tap.shape, ok.shape)
    return tap[ok]


def _rel(err: np.ndarray, ref: np.ndarray) -> np.ndarray:
    return err / np.maximum(ref, FLOOR * np.median(ref))


def tap_error(G, R) -> TapError:
    """The metrics of the module docstring for two (rows, D) matrices (``valid_rows`` makes them)."""
    G, R = _np(G).astype(np.float64), _np(R).astype(np.float64)
    assert G.shape == R.shape and G.ndim == 2, (G.shape, R.shape)
    if G.shape[0] == 0:
        return TapError(0, 0.0, 0.0, 0.0, 0.0, 0.0, -1, -1, 0.0)
    D = G - R
    rms = lambda x, ax: np.sqrt((x * x).mean(axis=ax))
    ch = _rel(rms(D, 0), rms(R, 0))
    row_rms = rms(D, 1)
    row = _rel(row_rms, rms(R, 1))
    row = np.where(np.isfinite(row), row, np.where(row_rms == 0, 0.0, np.inf))      # an all-zero reference: 0 / 0 -> 0
    ch = np.where(np.isfinite(ch), ch, np.where(rms(D, 0) == 0, 0.0, np.inf))
    return TapError(rows=int(G.shape[0]), max_ch=float(ch.max()), med_ch=float(np.median(ch)), max_row=float(row.max()),
                    med_row=float(np.median(row)), absmax=float(np.abs(D).max()), worst_ch=int(ch.argmax()), worst_row=int(row.argmax()),
                    max_row_rms=float(row_rms.max()))


def tap_error_padded(got, ref, mask, edge_index=None) -> TapError:
    """``tap_error`` of two padded taps over their valid rows."""
    return tap_error(valid_rows(got, mask, edge_index), valid_rows(ref, mask, edge_index))
