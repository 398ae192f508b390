"""Shared comparison helpers for the parity tests."""
import numpy as np

from oracle import pyoracle as po
from tools.simulate_reads import CAL_DIGITISATION, CAL_OFFSET, CAL_RANGE
from uncalled_amd import capi

HIT_INT_FIELDS = ("mapped", "fwd", "rd_st", "rd_en", "rd_len", "rf_st", "rf_en", "rf_len", "matches",
                  "n_events", "event_i", "n_nbr", "n_sa", "n_lf", "notes")


# Channel calibrations (range, offset, digitisation).  The simulators, the goldens and the example read all carry the first one; the others
# reach what it never does: another range with a small negative offset, a PromethION-like digitisation of 2048 with a large negative offset
# (illustrative values, not measured from a run), a non-integer offset, and identity (pA = the stored sample).  With an integer negative
# offset a stored -offset is exactly 0 pA and anything below it is negative.
REGIMES = {
    "minion": (CAL_RANGE, CAL_OFFSET, CAL_DIGITISATION),
    "minion_b": (1472.38, -7.0, 8192.0),
    "promethion": (748.6, -243.0, 2048.0),
    "frac_offset": (1398.7, 13.37, 8192.0),
    "identity": (8192.0, 0.0, 8192.0),
}


def calibrate_np(raw_i16, rng, offset, digitisation):
    """ReadBuffer's calibration restated in numpy float32: the stored int16 taken as u16, then add, multiply, divide, each rounded once."""
    u = np.asarray(raw_i16, dtype=np.int16).view(np.uint16).astype(np.float32)
    return (np.float32(rng) * (u + np.float32(offset))) / np.float32(digitisation)


def redigitise(raw_i16, from_cal, to_cal):
    """int16 samples recorded under `from_cal` -> the samples a channel calibrated with `to_cal` records for the same pA signal:
    rint(pA * digitisation / range - offset), kept inside [0, 32767]."""
    pa = calibrate_np(raw_i16, *from_cal).astype(np.float64)
    rng, offset, digit = to_cal
    return np.clip(np.rint(pa * digit / rng - offset), 0, 32767).astype(np.int16)


def calib_of(cals):
    """[(range, offset, digitisation)] -> CALIB array"""
    c = capi.make_calib(len(cals), 0.0, 0.0, 0.0)
    for i, (r, o, d) in enumerate(cals):
        c[i]["range"], c[i]["offset"], c[i]["digitisation"] = r, o, d
    return c


def oracle_hits(oix, raw, offsets, calib, params=None, fresh_mapper_per_read=False):
    """Map every read with the oracle restatement; returns O_HIT array."""
    out = np.zeros(offsets.size - 1, dtype=po.O_HIT)
    om = po.Mapper(oix, params)
    for i in range(offsets.size - 1):
        if fresh_mapper_per_read:
            om = po.Mapper(oix, params)
        sig = po.calibrate(raw[int(offsets[i]):int(offsets[i + 1])], float(calib["range"][i]),
                           float(calib["offset"][i]), float(calib["digitisation"][i]))
        out[i] = om.map_read(sig)
    return out


def assert_hits_equal(dev_hits, ora_hits, what=""):
    """Bit-exact: PAF coordinates, event counts and SURVEY 8(d) work counters; mean_event_len within 0 ulp."""
    assert len(dev_hits) == len(ora_hits)
    for i, (d, o) in enumerate(zip(dev_hits, ora_hits)):
        assert int(d["status"]) == 0, f"{what} read {i}: device status {int(d['status'])}"
        for f in HIT_INT_FIELDS:
            assert int(d[f]) == int(o[f]), f"{what} read {i}: {f} device={int(d[f])} oracle={int(o[f])}"
        if d["mapped"]:
            assert int(d["rid"]) == int(o["rid"]), f"{what} read {i}: rid"
            assert (int(d["cl_ref_st"]), int(d["cl_ref_en_start"]), int(d["cl_ref_en_end"]), int(d["cl_evt_st"]),
                    int(d["cl_evt_en"]), int(d["cl_total_len"])) == \
                   (int(o["cluster"]["ref_st"]), int(o["cluster"]["ref_en_start"]), int(o["cluster"]["ref_en_end"]),
                    int(o["cluster"]["evt_st"]), int(o["cluster"]["evt_en"]), int(o["cluster"]["total_len"])), \
                   f"{what} read {i}: cluster"
        assert np.float32(d["mean_event_len"]) == np.float32(o["mean_event_len"]) or int(o["n_events"]) == 0, \
            f"{what} read {i}: mean_event_len"


def to_oracle_params(p):
    """capi.Params -> pyoracle.Params (same field names)."""
    q = po.default_params()
    for name, _ in q._fields_:
        setattr(q, name, getattr(p, name))
    return q


def oracle_hits_threads(oix, raw, offsets, calib, dev_hits=None, threads=None):
    """The oracle on all host threads (po.map_batch: every thread ONE Mapper that maps read after read) for batches of thousands
    of reads.  A thread's Mapper carries sources_added_ from a read that filled max_paths into its next read (mapper.cpp:88,612-623),
    whichever read that happens to be; the device maps every read as a fresh Mapper does.  So a read that disagrees with `dev_hits`
    is mapped once more by a FRESH oracle Mapper before it counts (tests/dev/parity_sweep.py does the same against the reference)."""
    import os
    threads = threads or max(1, min(offsets.size - 1, len(os.sched_getaffinity(0))))
    sig = np.zeros(raw.size, dtype=np.float32)
    for i in range(offsets.size - 1):            # every read under its own calibration
        a, b = int(offsets[i]), int(offsets[i + 1])
        sig[a:b] = po.calibrate(raw[a:b], float(calib["range"][i]), float(calib["offset"][i]), float(calib["digitisation"][i]))
    want, secs = po.map_batch(oix, sig, offsets, threads)
    redone = 0
    if dev_hits is not None:
        for i in range(offsets.size - 1):
            if any(int(dev_hits[f][i]) != int(want[f][i]) for f in HIT_INT_FIELDS):
                want[i] = po.Mapper(oix).map_read(sig[int(offsets[i]):int(offsets[i + 1])])
                redone += 1
    return want, secs, redone
