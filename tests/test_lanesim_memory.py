"""Who owns the host library's device memory (uncalled_amd/csrc/unc_host.cpp), watched through the emulator's runtime: every
hipMalloc is given back, and an allocation that fails in the middle of a growth leaves a long-lived mapper usable.  The emulator
(tests/lanesim) counts the live allocations and can make the k-th next hipMalloc fail; the product sources know of neither."""
import ctypes as C
import gc
import itertools

import numpy as np
import pytest

from uncalled_amd import capi

pytestmark = pytest.mark.lanesim

UNC_ERR_HIP = -3     # include/uncalled_hip.h


def _live(lib):
    return C.c_int.in_dll(lib, "lanesim_live_allocs").value


def _arm(lib, k):
    """the k-th next hipMalloc fails (0: none does)"""
    C.c_int.in_dll(lib, "lanesim_fail_malloc_in").value = k


def _batch(example, n):
    raw = np.tile(example["signal"], n)
    off = np.arange(n + 1, dtype=np.uint64) * example["signal"].size
    return raw, off, capi.make_calib(n, example["range"], example["offset"], example["digitisation"])


def _chunk(example, read_number, n_samples):
    """the first chunk of a new read on channel 0"""
    ch = np.zeros(1, dtype=capi.RT_CHUNK)
    ch["channel"], ch["read_number"], ch["flags"], ch["n_samples"], ch["offset"] = 0, read_number, capi.RT_FIRST, n_samples, 0
    ch["calib"] = capi.make_calib(1, example["range"], example["offset"], example["digitisation"])[0]
    return ch


def _same(a, b):
    return all(np.array_equal(a[f], b[f]) for f in capi.RESULT_FIELDS)


def test_everything_is_given_back(sim_lib, example):
    """Every entry point that allocates device memory, once, and a unc_mapper_create that fails after its slots and its node pool
    exist: when everything is freed, no allocation is left."""
    gc.collect()
    start = _live(sim_lib)
    ix = capi.Index(example["prefix"], lib=sim_lib)
    assert _live(sim_lib) > start
    m = capi.Mapper(ix, n_slots=2, n_waves=2)
    raw, off, cal = _batch(example, 2)
    first = m.map_batch(raw, off, cal)
    assert first[0]["mapped"] and _same(first[0], first[1])
    m.set_read_order(capi.ORDER_T1)
    assert _same(m.map_batch(raw, off, cal), first)
    m.set_read_order(capi.ORDER_INDEPENDENT)
    mt = capi.Mapper(ix, n_slots=2, n_waves=2)       # (a trace reads slot 0 as a new mapper leaves it: a mapper of its own)
    assert len(list(itertools.islice(mt.trace(example["signal"], cal[:1]), 3))) == 3
    mt.trace_finish()
    rt = capi.Realtime(ix, n_channels=1)
    assert rt.process_chunks(_chunk(example, 1, 1000), raw_i16=example["signal"])[0]["state"] == capi.RT_MAPPING
    text = np.random.default_rng(5).integers(0, 4, size=300).astype(np.uint8)
    sa = capi.build_suffix_array(text, 0, sim_lib)
    assert sorted(sa.tolist()) == list(range(300))
    keys = np.random.default_rng(6).integers(0, 1 << 40, size=500, dtype=np.uint64)
    assert np.array_equal(capi.sort_pairs(keys, key_bits=40, lib=sim_lib)[0], np.sort(keys))
    a = np.zeros(6, dtype=np.uint64)
    sim_lib.unc_mapper_device_addresses.argtypes = [C.c_void_p, C.c_void_p]
    sim_lib.unc_calib_chase.argtypes = [C.c_int, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_void_p]
    assert sim_lib.unc_mapper_device_addresses(m.h, a.ctypes.data) == 0
    ms = C.c_float(-1.0)
    assert sim_lib.unc_calib_chase(0, int(a[0]), int(a[1]) * 2, 2, 16, C.byref(ms)) == 0 and ms.value >= 0.0
    # (five slots on two wavefronts want the sliced scheduler, whose seven parts do not divide them: refused after the slots and the pool)
    before = _live(sim_lib)
    with pytest.raises(capi.UncalledHipError, match="sched_parts"):
        capi.Mapper(ix, n_slots=5, n_waves=2, sched_parts=7)
    assert _live(sim_lib) == before
    rt.close()
    mt.close()
    m.close()
    ix.close()
    assert _live(sim_lib) == start


def test_failed_growth_leaves_the_mapper_usable(sim_lib, example):
    """A batch (a chunk round) larger than the last one grows the mapper's buffers.  Whichever of the growth's allocations fails, the
    call returns UNC_ERR_HIP and the mapper goes on mapping what it mapped before, with the same answer.

    Before the buffers owned their capacity this case wrote through a null pointer for some k: the buffers were freed and set to null,
    and the capacity beside them kept its old value when an allocation failed, so that the next smaller batch skipped the growth.

    (A chunk round has ONE allocation that grows -- the raw signal --, so there is one k to fail on the chunked path; a batch has
    seven: the raw signal, the five per-read arrays and the event means.)"""
    gc.collect()
    start = _live(sim_lib)
    ix = capi.Index(example["prefix"], lib=sim_lib)
    # (a pool of a given size: pool_fit, whose failed resizes are swallowed by design, stays out of the way)
    m = capi.Mapper(ix, n_slots=2, n_waves=2, pool_chunks=16)
    raw1, off1, cal1 = _batch(example, 1)
    raw2, off2, cal2 = _batch(example, 2)
    hits2 = np.zeros(2, dtype=capi.HIT)
    first = m.map_batch(raw1, off1, cal1)
    assert first[0]["mapped"]
    failed = 0
    for k in itertools.count(1):
        assert k < 100
        _arm(sim_lib, k)
        rc = sim_lib.unc_map_batch(m.h, 2, raw2.ctypes.data, off2.ctypes.data, cal2.ctypes.data, 0, None, hits2.ctypes.data)
        _arm(sim_lib, 0)
        if rc == 0:
            break
        assert rc == UNC_ERR_HIP, (k, rc, sim_lib.unc_last_error())
        failed += 1
        assert _same(m.map_batch(raw1, off1, cal1), first), k
    assert failed >= 3
    assert _same(hits2[0], first[0]) and _same(hits2[1], first[0])

    rt = capi.Realtime(ix, n_channels=1)
    sig = np.ascontiguousarray(example["signal"], dtype=np.int16)
    assert sig.size >= 3000
    res = np.zeros(1, dtype=capi.RT_RESULT)
    short = rt.process_chunks(_chunk(example, 1, 1000), raw_i16=sig)
    assert short[0]["state"] == capi.RT_MAPPING
    failed = 0
    for k in itertools.count(1):
        assert k < 100
        long_chunk = _chunk(example, 2 * k, 3000)
        _arm(sim_lib, k)
        rc = sim_lib.unc_rt_process_chunks(rt.h, 1, long_chunk.ctypes.data, sig.ctypes.data, 0, None, res.ctypes.data)
        _arm(sim_lib, 0)
        if rc == 0:
            break
        assert rc == UNC_ERR_HIP, (k, rc, sim_lib.unc_last_error())
        failed += 1
        again = rt.process_chunks(_chunk(example, 2 * k + 1, 1000), raw_i16=sig)
        assert again[0]["state"] == short[0]["state"] and _same(again[0]["hit"], short[0]["hit"]), k
    assert failed >= 1
    assert res[0]["state"] in (capi.RT_MAPPING, capi.RT_MAPPED)

    rt.close()
    m.close()
    ix.close()
    assert _live(sim_lib) == start


def test_chunk_after_a_failed_round_of_the_last_allowed_chunk(sim_lib, example):
    """The one way to Mapper::add_chunk's chunks_maxed() exit (mapper.cpp:289-296) in unc_rt_process_chunks: every call that maps a
    read's max_chunks-th chunk fails the read itself, unless the call dies on the device after the chunk was admitted -- here its
    growth of the raw-signal buffer fails.  The read's next chunk is then dropped: the read fails without being given up (not
    ENDED), its length is that of the chunks admitted so far, and the channel is free for a new read."""
    gc.collect()
    start = _live(sim_lib)
    ix = capi.Index(example["prefix"], lib=sim_lib)
    p = capi.default_params(sim_lib)
    p.max_chunks = 2
    rt = capi.Realtime(ix, n_channels=1, params=p)
    sig = np.ascontiguousarray(example["signal"], dtype=np.int16)
    assert sig.size >= 4000
    short = rt.process_chunks(_chunk(example, 1, 1000), raw_i16=sig)
    assert short[0]["state"] == capi.RT_MAPPING
    more = _chunk(example, 1, 3000)
    more["flags"], more["offset"] = 0, 1000
    res = np.zeros(1, dtype=capi.RT_RESULT)
    _arm(sim_lib, 1)
    rc = sim_lib.unc_rt_process_chunks(rt.h, 1, more.ctypes.data, sig.ctypes.data, 0, None, res.ctypes.data)
    _arm(sim_lib, 0)
    assert rc == UNC_ERR_HIP, (rc, sim_lib.unc_last_error())
    more["n_samples"] = 500
    dropped = rt.process_chunks(more, raw_i16=sig)[0]
    assert dropped["state"] == capi.RT_FAILED and not dropped["ended"] and not dropped["hit"]["mapped"]
    assert int(dropped["hit"]["rd_len"]) == int(np.float32(4000) * (np.float32(p.bp_per_sec) / np.float32(p.sample_rate)))
    assert int(dropped["hit"]["event_i"]) == int(short[0]["hit"]["event_i"]) and int(dropped["hit"]["n_events"]) == 0
    assert rt.process_chunks(more, raw_i16=sig)[0]["state"] == capi.RT_IGNORED
    again = rt.process_chunks(_chunk(example, 2, 1000), raw_i16=sig)
    assert again[0]["state"] == short[0]["state"] and _same(again[0]["hit"], short[0]["hit"])
    rt.close()
    ix.close()
    assert _live(sim_lib) == start


# hipMalloc calls of each creation on the example index, counted by the loop below on e40587f (the commit before the creations
# became plan / allocations / builds): the order and the number of a creation's allocations decide where its memory lies
# (DESIGN.md section 5), so a change of either must be meant
CREATION_ALLOCS = dict(index=10, index_bwa_sa=8, index_no_fm32=8, mapper=5, mapper_sliced=8, realtime=14)
INDEX_KNOBS = dict(index={}, index_bwa_sa={"UNC_DENSE_SA": "0"}, index_no_fm32={"UNC_FM32": "0"})
MAPPER_OPTS = dict(mapper=dict(n_slots=2, n_waves=2, pool_chunks=16),
                   # (sched_parts is named: xcd_count, which swallows a failed allocation and keeps its answer for the process, stays out)
                   mapper_sliced=dict(n_slots=64, n_waves=2, pool_chunks=16, sched_parts=1))


@pytest.mark.parametrize("what", list(CREATION_ALLOCS))
def test_creation_fails_clean_at_every_allocation(sim_lib, example, monkeypatch, what):
    """Whichever of a creation's allocations fails, the creation returns UNC_ERR_HIP and gives back what it had allocated; the first k
    at which it succeeds is one more than its number of allocations, which is the parent commit's.  The object then created maps the
    example read as one created undisturbed, and when everything is closed no allocation is left."""
    for k in ("UNC_DENSE_SA", "UNC_FM32", "UNC_WIDE_KEYS", "UNC_BUCKET_SHIFT", "UNC_RT_POOL_CHUNKS"):
        monkeypatch.delenv(k, raising=False)
    gc.collect()
    start = _live(sim_lib)
    raw, off, cal = _batch(example, 1)
    base_ix = capi.Index(example["prefix"], lib=sim_lib)
    want = capi.Mapper(base_ix, n_slots=2, n_waves=2, pool_chunks=16).map_batch(raw, off, cal)
    assert want[0]["mapped"]
    want_rt = capi.Realtime(base_ix, n_channels=1).process_chunks(_chunk(example, 1, 1000), raw_i16=example["signal"])
    gc.collect()
    for k, v in INDEX_KNOBS.get(what, {}).items():
        monkeypatch.setenv(k, v)

    def create():
        if what in INDEX_KNOBS:
            return capi.Index(example["prefix"], lib=sim_lib)
        if what in MAPPER_OPTS:
            return capi.Mapper(base_ix, **MAPPER_OPTS[what])
        return capi.Realtime(base_ix, n_channels=1)

    before = _live(sim_lib)
    failed = 0
    for k in itertools.count(1):
        assert k < 100
        _arm(sim_lib, k)
        try:
            obj = create()
            break
        except capi.UncalledHipError as e:
            assert str(e).startswith("uncalled_hip error %d:" % UNC_ERR_HIP), (k, e)
        finally:
            _arm(sim_lib, 0)
        failed += 1
        assert _live(sim_lib) == before, k
    print(what, "allocations:", failed)
    assert failed == CREATION_ALLOCS[what]

    if what in INDEX_KNOBS:
        m = capi.Mapper(obj, n_slots=2, n_waves=2, pool_chunks=16)
        assert _same(m.map_batch(raw, off, cal), want)
        m.close()
    elif what in MAPPER_OPTS:
        assert _same(obj.map_batch(raw, off, cal), want)
    else:
        got = obj.process_chunks(_chunk(example, 1, 1000), raw_i16=example["signal"])
        assert got[0]["state"] == want_rt[0]["state"] == capi.RT_MAPPING and _same(got[0]["hit"], want_rt[0]["hit"])
    obj.close()
    base_ix.close()
    assert _live(sim_lib) == start
