"""From the device's decision trace to the reference's ``analysis_data``.

``bpmx_beats_device_ex`` (csrc/bpmx_beats_core.h, ``beats_trace``) keeps, per
raw peak, the numbers ``beats.PeakClassifier._pair`` / ``._lone`` format into
their reason strings, a code that says which strings the peak has, and which
label each gap-fill pass of ``beats.fix_rhythmic_discontinuities`` gave it.
This module writes the strings from those numbers with the classifier's own
f-string formats, so identical doubles give identical text, and builds the
dict ``PeakClassifier.classify_peaks`` + ``refine_peaks`` leave behind:

* ``beat_debug_info``          {sample index: reason string} per raw peak
* ``long_term_bpm_series``     the belief after every classifier iteration
* ``deviation_series``         the smoothed amplitude deviation, main pass
* ``trough_indices`` / ``dynamic_noise_floor_series``  when the caller has them

No classifier runs here.  The Python route's ``KICK-START`` and ``CASCADE
RESET`` ``logging.info`` lines are not reproduced: they are log output, not
part of ``analysis_data`` or of any report.
"""
from __future__ import annotations

from typing import Dict, List, Optional

import numpy as np
import pandas as pd

from . import _native as N
from .beats import (LONE_S1, LONE_S1_CASCADE, LONE_S1_LAST, S1_GAP, S1_PAIRED, S2_GAP, S2_PAIRED)

NFIELDS = N.TR_NFIELDS
_GAP_LABEL = {N.TR_GAP_S1: S1_GAP, N.TR_GAP_S2: S2_GAP}
GAP_PASSES = 5


def _pair_text(r: List[float], code: int, thr: float) -> str:
    """PeakClassifier._pair's reason from one record."""
    why = f"Base Conf (Blended Model {r[N.TR_BLEND]:.0%} High): {r[N.TR_BASE_CONF]:.2f}"
    if code & N.TRF_STABILITY:
        why += f"\n- Stability Pre-Adjust: x{r[N.TR_STAB_FACTOR]:.2f} (Pairing Ratio: {r[N.TR_STAB_RATIO]:.0%})"
    if code & N.TRF_PENALIZED:
        why += (f"\n- PENALIZED by {r[N.TR_ADJ_AMOUNT]:.2f} (S2 Str. Ratio {r[N.TR_ADJ_RATIO]:.1f}x > "
                f"Expected {r[N.TR_ADJ_RMAX]:.1f}x)")
    elif code & N.TRF_BOOSTED:
        why += f"\n- BOOSTED by {r[N.TR_ADJ_AMOUNT]:.2f} (S1 Str. Ratio {r[N.TR_ADJ_RATIO]:.1f}x > S2)"
    if code & N.TRF_INTERVAL:
        why += (f"\n- Interval PENALTY by {r[N.TR_IV_AMOUNT]:.2f} (Interval {r[N.TR_IV_GAP]:.3f}s > "
                f"Max {r[N.TR_IV_CAP]:.3f}s)")
    conf = r[N.TR_FINAL]
    why += f"\n- Final Score: {conf:.2f} vs Threshold {thr:.2f} -> {'Paired' if conf >= thr else 'Not Paired'}"
    return why


def _lone_why(r: List[float]) -> str:
    return (f"Rhythm Fit={r[N.TR_L_RHYTHM]:.2f} (Interval {r[N.TR_L_RR]:.3f}s vs Expected "
            f"{r[N.TR_L_EXPECTED]:.3f}s), Amplitude Fit={r[N.TR_L_AMP]:.2f} (Strength Ratio {r[N.TR_L_RATIO]:.2f}x)")


def _reject_text(r: List[float], code: int, thr: float) -> str:
    if code & N.TRF_FORWARD:
        return f"Rejected Lone S1: Forward check failed (Implies {r[N.TR_L_IMPLIED]:.0f} BPM)"
    return f"Rejected Lone S1: Confidence {r[N.TR_L_CONF]:.2f} < Threshold {thr:.2f}. ({_lone_why(r)})"


def classifier_strings(rec, code, params: Dict) -> List[str]:
    """One reason string per raw peak, as ``classify_peaks`` leaves them
    (before any gap correction).  ``rec``: [n, NFIELDS] doubles, ``code``: [n]."""
    p = params
    thr = p['pairing_confidence_threshold']
    lthr = p.get("lone_s1_confidence_threshold", 0.6)
    wr, wa = p.get('lone_s1_rhythm_weight', 0.65), p.get('lone_s1_amplitude_weight', 0.35)
    rows = np.asarray(rec, dtype=np.float64).reshape(-1, NFIELDS).tolist()
    codes = np.asarray(code).tolist()
    out: List[str] = []
    for j, (r, c) in enumerate(zip(rows, codes)):
        kind = c & N.TR_OUTCOME
        if kind == N.TR_LAST_PEAK:
            out.append(LONE_S1_LAST)
        elif kind == N.TR_S1_PAIRED:
            out.append(f"{S1_PAIRED}§PAIRING_SUCCESS_REASON§{_pair_text(r, c, thr)}")
        elif kind == N.TR_S2_PAIRED:                    # its S1's reason, one table position back
            if j == 0 or (codes[j - 1] & N.TR_OUTCOME) != N.TR_S1_PAIRED:
                raise ValueError(f"trace: S2 at raw peak {j} without its S1")
            out.append(S2_PAIRED + out[j - 1][len(S1_PAIRED):])
        elif kind in (N.TR_LONE_VALID, N.TR_FIRST_BEAT, N.TR_CASCADE, N.TR_NOISE):
            fail = f"PAIRING_FAIL_REASON§{_pair_text(r, c, thr).lstrip(' |')}"
            if kind == N.TR_FIRST_BEAT:
                out.append(f"{LONE_S1}§{fail}§LONE_S1_VALIDATE_REASON§First beat")
            elif kind == N.TR_LONE_VALID:
                conf = r[N.TR_L_CONF]
                detail = (f"Validated Lone S1: Confidence {conf:.3f} >= Threshold {lthr:.2f}. ({_lone_why(r)}, "
                          f"Weights: Rhythm={wr:.2f}, Amplitude={wa:.2f}, Final={conf:.3f})")
                out.append(f"{LONE_S1}§{fail}§LONE_S1_VALIDATE_REASON§{detail}")
            else:
                rej = f"LONE_S1_REJECT_REASON§{_reject_text(r, c, lthr)}"
                out.append(f"{LONE_S1_CASCADE if kind == N.TR_CASCADE else 'Noise'}§{fail}§{rej}")
        else:
            raise ValueError(f"trace: raw peak {j} has no outcome (code {c})")
    return out


def apply_gap_history(strings: List[str], gap) -> List[str]:
    """The ``ORIGINAL_REASON`` wrapping of the gap-fill passes, in pass order: a
    pass wraps what the passes before it left."""
    g = np.asarray(gap)
    out = list(strings)
    for j in np.flatnonzero(g).tolist():
        v = int(g[j])
        for it in range(GAP_PASSES):
            label = _GAP_LABEL.get((v >> (2 * it)) & 3)
            if label:
                out[j] = f"{label}§ORIGINAL_REASON§{out[j]}"
    return out


def assemble(idx, sr: int, params: Dict, trace: Dict, troughs=None, floor=None) -> Dict:
    """``analysis_data`` of one recording, equal to the Python route's
    (``beats.analyze_recording``).  ``idx``: the raw peaks (sample indices);
    ``trace``: this recording's slices as a dict of ``record`` [n, NFIELDS],
    ``code`` [n], ``gap`` [n], ``lt_pos`` / ``lt_bpm`` [n_lt], ``dev_t`` /
    ``dev`` [n - 1].  ``troughs`` and ``floor`` (anything with the floor's
    values, e.g. a ``pd.Series`` over the recording) are passed through."""
    pk = np.asarray(idx, dtype=np.int64)
    n = len(pk)
    if n < 2:
        return {"beat_debug_info": {}}
    text = apply_gap_history(classifier_strings(trace["record"], trace["code"], params), trace["gap"])
    data: Dict = {}
    if floor is not None:
        data["dynamic_noise_floor_series"] = floor
    if troughs is not None:
        data["trough_indices"] = troughs
    data["deviation_series"] = pd.Series(np.asarray(trace["dev"], dtype=np.float64),
                                         index=np.asarray(trace["dev_t"], dtype=np.float64))
    data["beat_debug_info"] = dict(zip(pk, text))
    pos = np.asarray(trace["lt_pos"], dtype=np.int64)
    if len(pos):
        data["long_term_bpm_series"] = pd.Series(np.asarray(trace["lt_bpm"], dtype=np.float64), index=pk[pos] / sr)
    return data
