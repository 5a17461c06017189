"""Host side of bpmx_metrics_device: the dict ``beats.final_metrics`` returns,
built from the positions and values the device computed (csrc/
bpmx_metrics_core.h).  Nothing is recomputed here: timestamps and BPM values
are looked up in the curve at the positions the device reports."""
from __future__ import annotations

import datetime
from typing import Dict, List, Optional

import numpy as np
import pandas as pd

from . import _native as N
from . import beats as B

HRV_COLS = ['time', 'rmssdc', 'sdnn', 'bpm']
_UNIX = datetime.datetime(1970, 1, 1)


def epoch_us() -> int:
    """``beats._epoch()`` (the origin of the curve's index) in whole
    microseconds since 1970: 0 on a UTC machine."""
    d = B._epoch() - _UNIX
    return (d.days * 86400 + d.seconds) * 1000000 + d.microseconds


def curve_series(bpm_t: np.ndarray, bpm: np.ndarray) -> pd.Series:
    """The smoothed BPM curve as ``beats.bpm_series`` returns it."""
    if len(bpm) == 0:
        return pd.Series(dtype=np.float64)
    # epoch + timedelta(seconds=x) for the whole curve at once: CPython splits x with modf and rounds the
    # fraction's microseconds half to even (timedelta_us in csrc/bpmx_beats_core.h does the same)
    t = np.asarray(bpm_t, np.float64)
    whole = np.trunc(t)
    us = whole.astype(np.int64) * 1000000 + np.rint((t - whole) * 1e6).astype(np.int64)
    index = pd.DatetimeIndex(((epoch_us() + us) * 1000).view("M8[ns]"))
    return pd.Series(np.asarray(bpm, np.float64), index=index)


def _run(s: pd.Series, a: int, b: int, slope, dur, rising: bool) -> Dict:
    v0, v1 = s.values[a], s.values[b]
    d = {'start_time': s.index[a], 'end_time': s.index[b], 'start_bpm': v0, 'end_bpm': v1, 'duration_sec': float(dur)}
    d['bpm_increase' if rising else 'bpm_decrease'] = v1 - v0 if rising else v0 - v1
    d['slope_bpm_per_sec'] = np.float64(slope)
    return d


def _steepest(s: pd.Series, rec: np.ndarray) -> Optional[Dict]:
    if rec[0] != rec[0]:
        return None
    a, b = int(rec[0]), int(rec[1])
    return {'start_time': s.index[a], 'end_time': s.index[b], 'start_bpm': s.values[a], 'end_bpm': s.values[b],
            'slope_bpm_per_sec': np.float64(rec[2]), 'duration_sec': np.float64(rec[3])}


def record_of(m: Optional[Dict]):
    """(the 16-double record of bpmx_metrics_out, the HRV row count) of a
    ``final_metrics`` dict, however it was made: what ``shard.run_sharded``
    gathers per file.  None (no metrics) gives an all-NaN record."""
    rec = np.full(N.METRICS_RECORD, np.nan)
    if m is None:
        return rec, 0
    s = m['smoothed_bpm']
    ns = s.index.asi8 if len(s) else np.zeros(0, np.int64)
    pos = lambda ts: float(np.searchsorted(ns, pd.Timestamp(ts).value))  # noqa: E731
    for k, i in (('avg_bpm', N.MR_AVG_BPM), ('min_bpm', N.MR_MIN_BPM), ('max_bpm', N.MR_MAX_BPM),
                 ('avg_rmssdc', N.MR_AVG_RMSSDC), ('avg_sdnn', N.MR_AVG_SDNN)):
        if k in m['hrv_summary']:
            rec[i] = m['hrv_summary'][k]
    h = m['hrr_stats']
    if h is not None:
        rec[N.MR_HRR_PEAK:N.MR_HRR_PEAK + 3] = (pos(h['peak_time']), h['recovery_bpm'], h['hrr_value_bpm'])
    for k, i in (('peak_recovery_stats', N.MR_RECOVERY), ('peak_exertion_stats', N.MR_EXERTION)):
        d = m[k]
        if d is not None:
            rec[i:i + 4] = (pos(d['start_time']), pos(d['end_time']), d['slope_bpm_per_sec'], d['duration_sec'])
    return rec, len(m['windowed_hrv_df'])


def assemble(bpm_t: np.ndarray, bpm: np.ndarray, record: np.ndarray, hrv: Dict[str, np.ndarray],
             inc: Dict[str, np.ndarray], dec: Dict[str, np.ndarray], hrr_interval_sec: int = 60) -> Dict:
    """``beats.final_metrics``' dict from one file's device results: the curve,
    the 16-double record, the HRV columns (``time``, ``rmssdc``, ``sdnn``,
    ``bpm``) and the runs (``a``, ``b``, ``slope``, ``dur``)."""
    s = curve_series(bpm_t, bpm)
    m: Dict = {'smoothed_bpm': s, 'bpm_times': np.asarray(bpm_t, np.float64)}
    runs: List[List[Dict]] = []
    for r, rising in ((inc, True), (dec, False)):
        runs.append([_run(s, int(a), int(b), sl, du, rising)
                     for a, b, sl, du in zip(r["a"], r["b"], r["slope"], r["dur"])])
    m['major_inclines'], m['major_declines'] = runs
    hrr = None
    if record[N.MR_HRR_PEAK] == record[N.MR_HRR_PEAK]:
        am = int(record[N.MR_HRR_PEAK])
        hrr = {'peak_bpm': s.values[am], 'peak_time': s.index[am],
               'recovery_bpm': np.float64(record[N.MR_HRR_RECOVERY_BPM]),
               'recovery_check_time': s.index[am] + pd.Timedelta(seconds=hrr_interval_sec),
               'hrr_value_bpm': np.float64(record[N.MR_HRR_VALUE]), 'interval_sec': hrr_interval_sec}
    m['hrr_stats'] = hrr
    m['peak_recovery_stats'] = _steepest(s, record[N.MR_RECOVERY:N.MR_RECOVERY + 4])
    m['peak_exertion_stats'] = _steepest(s, record[N.MR_EXERTION:N.MR_EXERTION + 4])
    n = len(hrv["time"])
    m['windowed_hrv_df'] = (pd.DataFrame({c: np.asarray(hrv[c], np.float64) for c in HRV_COLS}) if n
                            else pd.DataFrame(columns=HRV_COLS))
    summ = {}
    if len(s):
        summ.update(avg_bpm=np.float64(record[N.MR_AVG_BPM]), min_bpm=np.float64(record[N.MR_MIN_BPM]),
                    max_bpm=np.float64(record[N.MR_MAX_BPM]))
    if n:
        summ.update(avg_rmssdc=np.float64(record[N.MR_AVG_RMSSDC]), avg_sdnn=np.float64(record[N.MR_AVG_SDNN]))
    m['hrv_summary'] = summ
    return m
