"""The realtime host classes (Chunk / RealtimePool / ClientSim of `_uncalled_amd`, mirroring src/chunk.hpp:47-59,
src/realtime_pool.hpp:63-70, src/client_sim.hpp:39-44) -- their sources linked against the lanesim build of the C ABI and
driven the way MapPoolOrd drives the reference's pool (map_pool_ord.cpp:61-112: try_add_chunk, an empty chunk once a read
has run out, update), checked read by read against the oracle's chunked path."""
from pathlib import Path

import numpy as np
import pytest

from tests.helpers import REGIMES, redigitise
from tools.simulate_reads import CAL_DIGITISATION, CAL_OFFSET, CAL_RANGE

G = Path(__file__).resolve().parent / "golden"
# a calibration for read i: the regimes in turn, one of them with more significant digits than a fast5 attribute keeps on its way
# through Fast5Reader (6: unc_pool.cpp attr_double)
_CALS = list(REGIMES.values()) + [(1472.3817, -7.0, 8192.0)]


def _read_cal(i):
    return _CALS[i % len(_CALS)]


def _as_read(cal):
    """the calibration Fast5Reader hands on for `cal` written into a fast5: each value as a float, printed with 6 significant digits"""
    return tuple(float(f"{float(np.float32(x)):.6g}") for x in cal)


def _sim_read(goldens, i, cal=None):
    """golden simulated read i, re-digitised for `cal` (default _read_cal(i))"""
    off = goldens["sim_offsets"]
    return redigitise(goldens["sim_signal"][int(off[i]):int(off[i + 1])], REGIMES["minion"], cal or _read_cal(i))


def case_chunk_class(unc):
    sig = [float(i) for i in range(10)]
    c = unc.Chunk("r1", 7, 3, 4000, sig, 2, 5)
    assert (c.id, c.channel, c.number, c.size(), c.empty(), c.start) == ("r1", 7, 3, 5, False, 4000)
    assert c.pop() == [2.0, 3.0, 4.0, 5.0, 6.0] and c.empty()
    assert unc.Chunk("r1", 7, 3, 0, sig, 8, 5).size() == 2                 # cut at the end of the read (chunk.cpp:60-66)
    raw = np.array([-3, 0, 700, 32767], dtype=np.int16)
    assert unc.Chunk("r", 1, 0, 0, "int16", raw.tobytes()).pop() == [-3.0, 0.0, 700.0, 32767.0]   # no calibration (chunk.cpp:33-38)
    f = np.array([1.5, -2.25], dtype=np.float32)
    assert unc.Chunk("r", 1, 0, 0, "float32", f.tobytes()).pop() == [1.5, -2.25]
    a, b = unc.Chunk("a", 1, 1, 0, sig, 0, 3), unc.Chunk("b", 2, 2, 9, sig, 0, 4)
    a.swap(b)
    assert (a.id, a.channel, a.number, a.size(), b.id, b.size()) == ("b", 2, 2, 4, "a", 3)


def _conf(unc, n_channels, **kw):
    c = unc.Conf()
    c.bwa_prefix = str(G / "example_index" / "example_ref")
    c.num_channels = n_channels
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def case_realtime_pool_ordered_replay(unc, po, example, goldens, n_reads=9):
    n_channels, chunk_len = 3, 4000
    off = goldens["sim_offsets"]
    reads = [po.calibrate(example["signal"], example["range"], example["offset"], example["digitisation"])]
    for i in range(n_reads - 1):                        # every read under a calibration of its own
        reads.append(po.calibrate(_sim_read(goldens, i), *_read_cal(i)))
    oix = po.Index(G / "example_index" / "example_ref")
    oms = [po.Mapper(oix) for _ in range(n_channels)]
    want = {i: oms[i % n_channels].chunk_read(reads[i], chunk_len)[0] for i in range(n_reads)}

    pool = unc.RealtimePool(_conf(unc, n_channels))
    queues = [[i for i in range(n_reads) if i % n_channels == ch] for ch in range(n_channels)]
    chunk_i = [0] * n_channels
    got = {}
    rounds = 0
    while any(queues) or not pool.all_finished():
        for ch, nm, paf in pool.update():
            i = nm
            got[i] = paf
            assert queues[ch - 1] and queues[ch - 1][0] == i
            queues[ch - 1].pop(0)
            chunk_i[ch - 1] = 0
        for ch in range(n_channels):                       # MapPoolOrd::update: the next chunk of the channel's front read
            if not queues[ch]:
                continue
            i = queues[ch][0]
            sig = reads[i]
            st = min(chunk_i[ch] * chunk_len, len(sig))
            c = unc.Chunk("read%d" % i, ch + 1, i, st, sig.tolist(), st, chunk_len)
            if pool.try_add_chunk(c):
                chunk_i[ch] += 1
        rounds += 1
        assert rounds < 2000
    names = oix.ref_names()
    assert sorted(got) == list(range(n_reads))
    for i in range(n_reads):
        cols = str(got[i]).split("\t")
        o = want[i]
        assert cols[0] == "read%d" % i
        wantcols = po.hit_paf_cols(o, names)
        if o["mapped"]:
            assert got[i].is_mapped()
            assert (int(cols[1]), int(cols[2]), int(cols[3]), cols[4], cols[5], int(cols[6]), int(cols[7]), int(cols[8]), int(cols[9]),
                    int(cols[10]), int(cols[11])) == wantcols, (i, cols, wantcols)
        else:
            assert not got[i].is_mapped() and int(cols[1]) == wantcols[0] and cols[2] == "*"
        assert "ch:i:%d" % (i % n_channels + 1) in cols
    pool.stop_all()
    assert pool.all_finished() and pool.update() == []


def case_add_chunk_resets_the_previous_read(unc, po, goldens):
    """RealtimePool::add_chunk (realtime_pool.cpp:74-110): a chunk of a NEW read on a channel whose read is still undecided
    ends that read (unmapped, `ended`) and starts the new one."""
    pool = unc.RealtimePool(_conf(unc, 2))
    noise = (np.random.default_rng(3).normal(90.0, 12.0, 9000)).astype(np.float32).tolist()      # never maps
    assert pool.add_chunk(unc.Chunk("noise", 1, 5, 100, noise, 0, 4000))
    assert not pool.add_chunk(unc.Chunk("noise", 1, 5, 4100, noise, 4000, 4000))                 # previous chunk not mapped yet
    assert pool.update() == [] and pool.active_count() == 1
    assert pool.add_chunk(unc.Chunk("noise", 1, 5, 4100, noise, 4000, 4000))
    assert pool.update() == []
    off = goldens["sim_offsets"]
    good = po.calibrate(goldens["sim_signal"][int(off[0]):int(off[1])], CAL_RANGE, CAL_OFFSET, CAL_DIGITISATION).tolist()
    assert pool.add_chunk(unc.Chunk("good", 1, 6, 0, good, 0, 4000))                              # new read number on channel 1
    out = pool.update()
    ended = [(ch, nm, p) for ch, nm, p in out if nm == 5]
    assert len(ended) == 1 and ended[0][0] == 1 and ended[0][2].is_ended() and not ended[0][2].is_mapped()
    assert str(ended[0][2]).split("\t")[0] == "noise" and int(str(ended[0][2]).split("\t")[1]) == int(8000 * 450.0 / 4000.0)
    k = 1
    mapped = [p for ch, nm, p in out if nm == 6]
    while not mapped and k * 4000 < len(good):
        assert pool.add_chunk(unc.Chunk("good", 1, 6, k * 4000, good, k * 4000, 4000))
        mapped = [p for ch, nm, p in pool.update() if nm == 6]
        k += 1
    assert mapped and mapped[0].is_mapped() and pool.all_finished()


def case_oversized_chunk_is_refused(unc):
    """A chunk longer than chunk_time * sample_rate (a client on another chunk time) is refused by add_chunk / try_add_chunk
    and leaves the pool running: the reference's ReadBuffer would append it, the device side stages one chunk_len per
    channel, and one bad chunk must not end the run."""
    pool = unc.RealtimePool(_conf(unc, 2))
    noise = (np.random.default_rng(4).normal(90.0, 12.0, 12000)).astype(np.float32).tolist()
    assert not pool.add_chunk(unc.Chunk("big", 1, 1, 0, noise, 0, 4001))
    assert not pool.try_add_chunk(unc.Chunk("big", 1, 1, 0, noise, 0, 8000))
    assert pool.update() == [] and pool.active_count() == 0 and pool.all_finished()
    assert pool.refused_chunks() == 2
    assert pool.add_chunk(unc.Chunk("ok", 1, 2, 0, noise, 0, 4000))           # the channel still takes a regular chunk
    assert pool.update() == [] and pool.active_count() == 1
    # ... and an oversized one mid-read is refused AND ends the read (unmapped + ended at the next update): the channel is free again
    assert not pool.add_chunk(unc.Chunk("ok", 1, 2, 4000, noise, 4000, 5000))
    assert pool.active_count() == 0 and pool.refused_chunks() == 3
    out = pool.update()
    assert len(out) == 1 and out[0][0] == 1 and out[0][1] == 2 and out[0][2].is_ended() and not out[0][2].is_mapped()
    assert str(out[0][2]).split("\t")[0] == "ok" and int(str(out[0][2]).split("\t")[1]) == int(4000 * 450.0 / 4000.0)
    assert pool.all_finished()
    assert pool.add_chunk(unc.Chunk("next", 1, 3, 0, noise, 0, 4000)) and pool.active_count() == 1
    # two reads given up on ONE channel between two updates (round-4 advice): read 3 is mapping; a chunk of read 4 takes the channel
    # over (3 is reset); an oversized chunk of read 4 arrives before update() and ends 4 as well.  Both get their unmapped + ended line
    # -- the reference reports every reset read (a single give-up record per channel lost read 3's)
    assert pool.update() == [] and pool.active_count() == 1
    assert pool.add_chunk(unc.Chunk("four", 1, 4, 0, noise, 0, 4000))
    assert not pool.add_chunk(unc.Chunk("four", 1, 4, 4000, noise, 4000, 5000))
    out = pool.update()
    assert sorted((ch, nm, str(p).split("\t")[0], p.is_ended(), p.is_mapped()) for ch, nm, p in out) == \
        [(1, 3, "next", True, False), (1, 4, "four", True, False)]
    assert pool.all_finished() and pool.update() == []


def case_channel_transitions(unc, po, goldens):
    """The rows of RealtimePool's channel table (unc_realtime.hpp) that no other case reaches: end_read in every state, the empty
    chunk of try_add_chunk, a foreign read number in try_add_chunk, an oversized chunk on a channel that does not exist, stop_all."""
    pool = unc.RealtimePool(_conf(unc, 2))
    noise = (np.random.default_rng(5).normal(90.0, 12.0, 8000)).astype(np.float32).tolist()      # never maps
    empty = lambda rid, ch, nm: unc.Chunk(rid, ch, nm, len(noise), noise, len(noise), 4000)      # past the read's end: no samples
    assert empty("a", 1, 1).empty()

    def unmapped_ended(out, ch, nm, rid, raw_len):
        assert len(out) == 1 and out[0][:2] == (ch, nm) and out[0][2].is_ended() and not out[0][2].is_mapped()
        assert str(out[0][2]).split("\t")[:2] == [rid, str(int(raw_len * 450.0 / 4000.0))]

    # end_read on a read that is mapping: unmapped + ended at the next update; a wrong number or a channel past the end: nothing
    assert pool.add_chunk(unc.Chunk("a", 1, 1, 0, noise, 0, 4000))
    assert pool.update() == [] and pool.active_count() == 1
    pool.end_read(0, 2)
    pool.end_read(1, 1)
    pool.end_read(2, 1)
    pool.end_read(65535, 1)
    assert pool.active_count() == 1 and pool.update() == [] and not pool.all_finished()
    pool.end_read(0, 1)
    assert pool.active_count() == 0 and not pool.all_finished()
    unmapped_ended(pool.update(), 1, 1, "a", 4000)
    assert pool.all_finished() and pool.update() == []
    # a read whose first chunk is still only pending: an empty chunk changes nothing, end_read makes it vanish with no record
    assert pool.add_chunk(unc.Chunk("b", 1, 2, 0, noise, 0, 4000))
    assert not pool.try_add_chunk(empty("b", 1, 2)) and pool.active_count() == 1
    pool.end_read(0, 2)
    assert pool.active_count() == 0 and pool.all_finished() and pool.update() == []
    # try_add_chunk, an empty chunk: nothing while a chunk is pending; once that one is mapped the read is given up, one record
    assert pool.try_add_chunk(unc.Chunk("c", 2, 3, 0, noise, 0, 4000))
    assert pool.update() == []
    assert pool.try_add_chunk(unc.Chunk("c", 2, 3, 4000, noise, 4000, 4000))
    assert not pool.try_add_chunk(empty("c", 2, 3)) and pool.active_count() == 1
    assert pool.update() == [] and pool.active_count() == 1
    assert not pool.try_add_chunk(unc.Chunk("d", 2, 4, 0, noise, 0, 4000))                       # another read: refused, nothing changes
    assert pool.active_count() == 1 and pool.update() == [] and not pool.all_finished()
    assert not pool.try_add_chunk(empty("c", 2, 3))
    assert pool.active_count() == 0 and not pool.all_finished()
    unmapped_ended(pool.update(), 2, 3, "c", 8000)
    assert pool.all_finished()
    # an oversized chunk on a channel past num_channels: add_chunk counts it as refused, try_add_chunk does not
    assert not pool.add_chunk(unc.Chunk("big", 3, 9, 0, noise, 0, 4001)) and pool.refused_chunks() == 1
    assert not pool.try_add_chunk(unc.Chunk("big", 3, 9, 0, noise, 0, 4001)) and pool.refused_chunks() == 1
    assert not pool.add_chunk(unc.Chunk("far", 3, 9, 0, noise, 0, 4000)) and not pool.try_add_chunk(unc.Chunk("far", 3, 9, 0, noise, 0, 4000))
    assert pool.refused_chunks() == 1 and pool.all_finished() and pool.update() == []
    # try_add_chunk with another read's chunk between the chunks of a read that goes on to map: that read is not disturbed
    off = goldens["sim_offsets"]
    good = po.calibrate(goldens["sim_signal"][int(off[0]):int(off[1])], CAL_RANGE, CAL_OFFSET, CAL_DIGITISATION).tolist()
    assert pool.try_add_chunk(unc.Chunk("good", 1, 6, 0, good, 0, 4000))
    assert not pool.try_add_chunk(unc.Chunk("other", 1, 7, 0, noise, 0, 4000))                   # ... while the first chunk is pending
    out, k = pool.update(), 1
    while not out and k * 4000 < len(good):
        assert not pool.try_add_chunk(unc.Chunk("other", 1, 7, 0, noise, 0, 4000))               # ... and while the read is mapping
        assert pool.try_add_chunk(unc.Chunk("good", 1, 6, k * 4000, good, k * 4000, 4000))
        out, k = pool.update(), k + 1
    assert len(out) == 1 and out[0][:2] == (1, 6) and out[0][2].is_mapped() and str(out[0][2]).split("\t")[0] == "good"
    assert pool.all_finished()
    # stop_all: nothing is taken and nothing is reported any more, not even a read given up just before
    assert pool.add_chunk(unc.Chunk("e", 2, 8, 0, noise, 0, 4000))
    assert pool.update() == [] and pool.active_count() == 1
    pool.end_read(1, 8)
    assert not pool.all_finished()
    pool.stop_all()
    assert not pool.add_chunk(unc.Chunk("f", 1, 9, 0, noise, 0, 4000)) and not pool.try_add_chunk(unc.Chunk("f", 1, 9, 0, noise, 0, 4000))
    assert not pool.add_chunk(unc.Chunk("f", 1, 9, 0, noise, 0, 4001)) and pool.refused_chunks() == 1
    assert pool.update() == [] and pool.active_count() == 0 and pool.all_finished()


def case_client_sim_feeds_the_decision_loop(unc, po, tmp_path, goldens):
    """ClientSim-shaped source over fast5 files + the enrich/deplete loop of scripts/uncalled:216-256 (uncalled_amd sim)."""
    off = goldens["sim_offsets"]
    cals = [_read_cal(i + 3) for i in range(4)]          # (the one with seven significant digits among them)
    reads = [dict(id="sim-%d" % i, channel=1 + i % 2, number=i, start=1000 * i, range=cals[i][0], offset=cals[i][1], digitisation=cals[i][2],
                  signal=_sim_read(goldens, i, cals[i]).tolist()) for i in range(4)]
    f5 = tmp_path / "reads.fast5"
    assert unc.write_fast5(str(f5), reads, True, 4000.0)
    conf = _conf(unc, 2)
    client = unc.ClientSim(conf)
    client.add_fast5(str(f5))
    client.load_fast5s()
    assert client.run() and client.is_running
    first = client.get_read_chunks()
    assert [(ch, c.id, c.number, c.size()) for ch, c in first] == [(1, "sim-0", 0, 4000), (2, "sim-1", 1, 4000)]
    assert first[0][1].start == 0 and first[1][1].start == 1000
    for k, (ch, c) in enumerate(first):                 # calibrated with the read's own calibration, as Fast5Reader reads it back
        want = po.calibrate(np.array(reads[k]["signal"][:4000], dtype=np.int16), *_as_read(cals[k]))
        assert np.array_equal(np.array(c.pop(), dtype=np.float32).view(np.uint32), want.view(np.uint32)), k
    client.stop_receiving_read(1, 0)                       # channel 1 moves on to its next read
    second = client.get_read_chunks()
    assert [(ch, c.id, c.start) for ch, c in second] == [(1, "sim-2", 2000), (2, "sim-1", 1000 + 4000)]
    assert client.unblock_read(2, 1) == 0
    assert [(ch, c.id) for ch, c in client.get_read_chunks()] == [(1, "sim-2"), (2, "sim-3")]
    assert abs(client.get_runtime() - 3.0) < 1e-6

    from uncalled_amd.__main__ import realtime_loop
    lines = []
    conf.realtime_mode = int(unc.RealtimePool.DEPLETE)
    client = unc.ClientSim(conf)
    client.add_fast5(str(f5))
    client.load_fast5s()
    client.run()
    pool = unc.RealtimePool(conf)
    realtime_loop(unc, conf, client, pool, sim=True, emit=lambda p: lines.append(str(p)), sleep=lambda s: None)
    ids = sorted(l.split("\t")[0] for l in lines)
    assert ids == ["sim-0", "sim-1", "sim-2", "sim-3"]
    for l in lines:      # deplete: mapped reads are ejected, unmapped ones kept
        assert ("\tej:f:" in l) == (l.split("\t")[2] != "*") and (("\tkp:f:" in l) or ("\ten:f:" in l) or ("\tej:f:" in l))


def case_map_pool_pipeline(unc, po, tmp_path, goldens):
    """MapPool (loader thread -> page-locked staging buffers -> mapper thread -> update()) over several fast5 files and
    batches: every read comes out once, PAF columns as the oracle maps the same signal."""
    off = goldens["sim_offsets"]
    n = 7
    # a calibration per read.  Mapping hardly depends on it (the detector's t-statistics and the normaliser undo an affine map of the
    # signal), except where event means leave [min_mean, max_mean]: each batch opens with the PromethION-like read, under whose
    # calibration the others' samples are negative pA -- a batch staged with its first read's calibration maps them to nothing
    mp = [REGIMES["promethion"], REGIMES["identity"], (1999.9375, 0.0, 2000.0)]       # (1999.9375: more digits than a fast5 keeps)
    cals = [mp[i % 3] for i in range(n - 1)] + [REGIMES["minion"]]
    reads = [dict(id="sim-%d" % i, channel=1 + i, number=i, start=100 * i, range=cals[i][0], offset=cals[i][1],
                  digitisation=cals[i][2], signal=_sim_read(goldens, i, cals[i]).tolist()) for i in range(n)]
    assert unc.write_fast5(str(tmp_path / "a.fast5"), reads[:4], True, 4000.0)
    assert unc.write_fast5(str(tmp_path / "b.fast5"), reads[4:6], True, 4000.0)
    assert unc.write_fast5(str(tmp_path / "c.fast5"), reads[6:], True, 4000.0)
    pool = unc.MapPool(_conf(unc, 512, batch_reads=3))          # 3 + 3, later 1
    pool.add_fast5(str(tmp_path / "a.fast5"))
    pool.add_fast5(str(tmp_path / "b.fast5"))
    assert pool.running()
    lines = []
    import time
    t0 = time.time()
    while pool.running():
        lines += [str(p) for p in pool.update()]
        time.sleep(0.01)
        assert time.time() - t0 < 600
    assert len(lines) == 6
    # the worker threads live until stop() (map_pool.cpp:31-42,83-97): a file added after the pool ran dry is mapped too
    pool.add_fast5(str(tmp_path / "c.fast5"))
    assert pool.running()
    while pool.running():
        lines += [str(p) for p in pool.update()]
        time.sleep(0.01)
        assert time.time() - t0 < 600
    pool.stop()
    assert not pool.running() and pool.update() == []
    oix = po.Index(G / "example_index" / "example_ref")
    om = po.Mapper(oix)
    got = {l.split("\t")[0]: l.split("\t") for l in lines}
    assert sorted(got) == sorted(r["id"] for r in reads) and len(lines) == n
    n_mapped = 0
    for i, r in enumerate(reads):
        o = om.map_read(po.calibrate(np.array(r["signal"], dtype=np.int16), *_as_read(cals[i])))
        want = po.hit_paf_cols(o, oix.ref_names())
        c = got[r["id"]]
        if o["mapped"]:
            assert c[2] != "*", (r["id"], "unmapped; the oracle maps it")
            assert (int(c[1]), int(c[2]), int(c[3]), c[4], c[5], int(c[6]), int(c[7]), int(c[8]), int(c[9]), int(c[10]), int(c[11])) == want
            n_mapped += 1
        else:
            assert int(c[1]) == want[0] and c[2] == "*"
        assert "ch:i:%d" % r["channel"] in c and "st:i:%d" % r["start"] in c
    assert n_mapped >= n - 2


def case_map_pool_short_of_staging_memory(unc, po, tmp_path, goldens, monkeypatch):
    """The loader with a staging buffer that cannot grow (round-3 advice: a read dropped without a PAF line, and a failed first
    read ending the run).  UNC_STAGING_MAX_KB caps a buffer at 40 KB = 20 000 samples: a batch that is full is handed over and the
    read that did not fit OPENS THE NEXT ONE; a read larger than the cap gets its unmapped line (length column as the reference
    prints it) and the run goes on.  Every read comes out exactly once, the staged ones with the oracle's columns."""
    import time
    monkeypatch.setenv("UNC_STAGING_MAX_KB", "40")
    off = goldens["sim_offsets"]
    n = 6
    reads = [dict(id="sim-%d" % i, channel=1 + i, number=i, start=100 * i, range=CAL_RANGE, offset=CAL_OFFSET, digitisation=CAL_DIGITISATION,
                  signal=goldens["sim_signal"][int(off[i]):int(off[i + 1])].tolist()[:9000]) for i in range(n)]
    big = dict(reads[2], id="too-big", signal=(reads[2]["signal"] * 4)[:30000])      # 60 KB: no buffer will ever hold it
    order = [big] + reads[:3] + [dict(big, id="too-big-2")] + reads[3:]                # ... also as the very first read of the run
    assert unc.write_fast5(str(tmp_path / "a.fast5"), order, True, 4000.0)
    pool = unc.MapPool(_conf(unc, 512, batch_reads=8))
    pool.add_fast5(str(tmp_path / "a.fast5"))
    lines, t0 = [], time.time()
    while pool.running():
        lines += [str(p) for p in pool.update()]
        time.sleep(0.01)
        assert time.time() - t0 < 600
    pool.stop()
    got = {l.split("\t")[0]: l.split("\t") for l in lines}
    assert len(lines) == len(order) and sorted(got) == sorted(r["id"] for r in order)
    for name in ("too-big", "too-big-2"):
        assert got[name][2] == "*" and int(got[name][1]) == int(np.float32(30000) * (np.float32(450.0) / np.float32(4000.0)))
    oix = po.Index(G / "example_index" / "example_ref")
    om = po.Mapper(oix)
    for r in reads:
        o = om.map_read(po.calibrate(np.array(r["signal"], dtype=np.int16), CAL_RANGE, CAL_OFFSET, CAL_DIGITISATION))
        want = po.hit_paf_cols(o, oix.ref_names())
        c = got[r["id"]]
        if o["mapped"]:
            assert (int(c[1]), int(c[2]), int(c[3]), c[4], c[5], int(c[6]), int(c[7]), int(c[8]), int(c[9]), int(c[10]), int(c[11])) == want
        else:
            assert int(c[1]) == want[0] and c[2] == "*"


# ---- the cases above on the lanesim build of the host module (tests/test_gpu_host.py runs them on the real one)
@pytest.mark.lanesim
def test_chunk_class(sim_host):
    case_chunk_class(sim_host)


@pytest.mark.lanesim
def test_realtime_pool_ordered_replay_matches_oracle(sim_host, oracle_lib, example, goldens):
    case_realtime_pool_ordered_replay(sim_host, oracle_lib, example, goldens, n_reads=5)     # 9 on the GPU


@pytest.mark.lanesim
def test_add_chunk_resets_the_previous_read(sim_host, oracle_lib, goldens):
    case_add_chunk_resets_the_previous_read(sim_host, oracle_lib, goldens)


@pytest.mark.lanesim
def test_oversized_chunk_is_refused(sim_host):
    case_oversized_chunk_is_refused(sim_host)


@pytest.mark.lanesim
def test_channel_transitions(sim_host, oracle_lib, goldens):
    case_channel_transitions(sim_host, oracle_lib, goldens)


@pytest.mark.lanesim
def test_client_sim_feeds_the_decision_loop(sim_host, oracle_lib, tmp_path, goldens):
    case_client_sim_feeds_the_decision_loop(sim_host, oracle_lib, tmp_path, goldens)


@pytest.mark.lanesim
def test_map_pool_pipeline_matches_oracle(sim_host, oracle_lib, tmp_path, goldens):
    case_map_pool_pipeline(sim_host, oracle_lib, tmp_path, goldens)


@pytest.mark.lanesim
def test_map_pool_short_of_staging_memory(sim_host, oracle_lib, tmp_path, goldens, monkeypatch):
    case_map_pool_short_of_staging_memory(sim_host, oracle_lib, tmp_path, goldens, monkeypatch)
