"""`python -m uncalled_amd {index,map,sim,dtw,mask,pafstats}` -- the subcommands of the reference's `scripts/uncalled` that do not need
a sequencer (index_cmd :38-78, map_cmd :126-167, realtime_cmd :170-256 fed from fast5 files, pafstats) with the same options (uncalled/args.py:90-124,244-304) on the GPU path.
"""
import argparse
import os
import sys
import time

MAX_SLEEP = 0.01
BWA_SUFFS = (".amb", ".ann", ".bwt", ".pac", ".sa")


def _assert_exists(fname):
    if not os.path.exists(fname):
        sys.stderr.write("Error: '%s' does not exist\n" % fname)
        sys.exit(1)


def load_fast5s(paths, recursive):
    """scripts/uncalled:80-119: directories (optionally recursive), .fast5 files, or text files of file names."""
    def keep(path):
        if path.startswith("#") or not path.endswith("fast5"):
            return None
        path = os.path.abspath(path)
        if not os.path.isfile(path):
            sys.stderr.write("Warning: \"%s\" is not a fast5 file.\n" % path)
            return None
        return path

    for path in paths:
        path = path.strip()
        if not os.path.exists(path):
            sys.stderr.write("Error: \"%s\" does not exist\n" % path)
            sys.exit(1)
        if os.path.isdir(path):
            if recursive:
                for root, _, files in os.walk(path):
                    for f in files:
                        yield keep(os.path.join(root, f))
            else:
                for f in os.listdir(path):
                    yield keep(os.path.join(path, f))
        elif path.endswith(".fast5"):
            yield keep(path)
        else:
            with open(path) as fh:
                for line in fh:
                    yield keep(line.strip())


def index_cmd(args):
    from . import capi, index_params
    prefix = args.bwa_prefix or args.fasta_filename
    if all(os.path.exists(prefix + s) for s in BWA_SUFFS):
        sys.stderr.write("Using previously built BWA index.\nNote: to fully re-build the index delete files with the "
                         "\"%s.*\" prefix.\n" % prefix)
    else:
        # the suffix sort inside bwa_idx_build (bwa_index.hpp:92-101) runs on the GPU behind the C ABI (unc_build_suffix_array: no torch
        # in the process) for references of fewer than 2^30 bases; larger ones go through the chunked builder (torch tensors around the
        # same radix sort)
        from . import build_index
        names, annos, seqs = build_index.read_fasta(args.fasta_filename)
        if 2 * sum(len(s) for s in seqs) < (1 << 31):
            codes, holes, n_ambs = build_index.encode_contigs(seqs)
            build_index.build_from_codes(prefix, names, annos, [len(s) for s in seqs], codes, holes, n_ambs, verbose=True,
                                         sa_device="cuda:%d" % args.device)
        else:
            from . import build_index_big
            codes, holes, n_ambs = build_index.encode_contigs(seqs)
            build_index_big.build_from_codes_big(prefix, names, annos, [len(s) for s in seqs], codes, holes, n_ambs, device="cuda:%d" % args.device)
    sys.stderr.write("Initializing parameter search\n")
    presets = [("default", dict(tgt_speed=115))]
    for tgt in (args.probs.split(",") if args.probs else []):
        presets.append(("prob_%s" % tgt, dict(tgt_prob=float(tgt))))
    for tgt in (args.speeds.split(",") if args.speeds else []):
        presets.append(("speed_%s" % tgt, dict(tgt_speed=float(tgt))))
    # the loader wants a preset (self-alignment does not read the thresholds): a placeholder .uncl lives only for the
    # duration of the search and never survives a failed or interrupted one -- `map` would load it silently
    placeholder = not os.path.exists(prefix + ".uncl")
    if placeholder:
        with open(prefix + ".uncl", "w") as f:
            f.write("default\t-10.0\t0.00000\t0.000\n")
    done = False
    try:
        ix = capi.Index(prefix, device=args.device)
        index_params.parameterize(ix, prefix, presets=presets, max_sample_dist=args.max_sample_dist,
                                  min_samples=args.min_samples, max_samples=args.max_samples, kmer_len=args.kmer_len,
                                  matchpr1=args.matchpr1, matchpr2=args.matchpr2,
                                  pathlen_percentile=args.pathlen_percentile, max_replen=args.max_replen)
        done = True
    finally:
        if placeholder and not done and os.path.exists(prefix + ".uncl"):
            os.unlink(prefix + ".uncl")
    sys.stderr.write("Done\n")


def shard_files(files, n_shards):
    """fast5 files of shard i = every n-th file starting at i: files (reads) are independent units, no exchange"""
    files = [f for f in files if f is not None]
    return [files[i::n_shards] for i in range(n_shards)]


def worker_cmd(args, list_name, dev):
    """command line of one `--gpus N` worker: everything but `-n`, which is a cap on the whole job (see map_multi_gpu)"""
    cmd = [sys.executable, "-m", "uncalled_amd", "map", args.bwa_prefix, list_name, "--device", str(dev), "--gpus", "1"]
    for opt, val in (("-p", args.idx_preset), ("-l", args.read_list), ("-e", args.max_events),
                     ("-c", args.max_chunks), ("--chunk-time", args.chunk_time), ("--batch-reads", args.batch_reads),
                     ("--model", getattr(args, "model_path", None))):
        if val is not None:
            cmd += [opt, str(val)]
    return cmd


def map_multi_gpu(args, argv, make_cmd=worker_cmd):
    """`map --gpus N`: one worker process per GPU (index replicated, fast5 files dealt round-robin), PAF lines of all
    workers forwarded to stdout as they come.  SURVEY 8(e): no collective, no data-path communication.
    `-l` goes to every worker in full (a worker only sees its own files, so each read id matches in one of them);
    `-n` is a cap on the whole job and is applied HERE, on the forwarded lines: workers are stopped once it is reached."""
    import subprocess
    import tempfile
    import threading
    shards = [x for x in shard_files(list(load_fast5s(args.fast5s, args.recursive)), args.gpus) if x]
    procs, lists = [], []
    lock = threading.Lock()
    state = {"n": 0, "full": False}
    limit = args.max_reads

    def pump(p):
        for line in p.stdout:
            with lock:
                if limit is not None and state["n"] >= limit:
                    state["full"] = True
                    break
                sys.stdout.write(line)
                state["n"] += 1
        p.stdout.close()

    try:
        for dev, files in enumerate(shards):
            lst = tempfile.NamedTemporaryFile("w", suffix=".fast5s.txt", delete=False)
            lists.append(lst.name)
            lst.write("\n".join(files) + "\n")
            lst.close()
            # UNC_PIN_WORLD: the worker keeps its host threads (HDF5 loader, staging, PAF writer) on its GPU's NUMA node
            procs.append(subprocess.Popen(make_cmd(args, lst.name, dev), stdout=subprocess.PIPE, text=True, bufsize=1,
                                          env={**os.environ, "UNC_PIN_WORLD": str(len(shards))}))
        threads = [threading.Thread(target=pump, args=(p,)) for p in procs]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        if state["full"]:
            for p in procs:
                if p.poll() is None:
                    p.terminate()
        codes = [p.wait() for p in procs]
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
        for name in lists:
            if os.path.exists(name):
                os.unlink(name)
    sys.stdout.flush()
    if any(codes) and not state["full"]:
        sys.stderr.write("Error: worker exit codes %s\n" % codes)
        sys.exit(1)


def map_cmd(args):
    if getattr(args, "gpus", 1) > 1:
        return map_multi_gpu(args, sys.argv)
    from . import _uncalled_amd as unc
    conf = unc.Conf()
    for k, v in vars(args).items():
        if v is not None and not k.startswith("_") and hasattr(conf, k):
            setattr(conf, k, v)
    _assert_exists(conf.bwa_prefix + ".bwt")
    _assert_exists(conf.bwa_prefix + ".uncl")
    if conf.model_path:
        _assert_exists(conf.model_path)
    if conf.read_list:
        _assert_exists(conf.read_list)
    pin_world = int(os.environ.get("UNC_PIN_WORLD", "0") or 0)
    if pin_world > 1:
        from .numa import pin_to_gpu_node
        sys.stderr.write("GPU %d: host threads -> %s\n" % (args.device, pin_to_gpu_node(args.device, pin_world)))
    mapper = unc.MapPool(conf)
    sys.stderr.write("Loading fast5s\n")
    for f in load_fast5s(args.fast5s, args.recursive):
        if f is not None:
            mapper.add_fast5(f)
    sys.stderr.write("Mapping\n")
    sys.stderr.flush()
    try:
        while mapper.running():
            t0 = time.time()
            for p in mapper.update():
                p.print_paf()
            dt = time.time() - t0
            if dt < MAX_SLEEP:
                time.sleep(MAX_SLEEP - dt)
    except KeyboardInterrupt:
        pass
    sys.stderr.write("Finishing\n")
    mapper.stop()


class _Channel:
    """What the decision session remembers about one channel."""
    __slots__ = ("last_chunk_at", "ejected_read")

    def __init__(self, now):
        self.last_chunk_at = now        # when the channel's newest chunk was handed to the pool (decision latency is taken from it)
        self.ejected_read = None        # number of the read this channel was told to eject: its late chunks are dropped


class RealtimeSession:
    """ReadUntil decisions over a RealtimePool and a chunk source with the ClientSim surface: the behaviour of the reference's
    `uncalled realtime / sim` main loop (scripts/uncalled:216-256 -- the caller of this repo's boundary, not part of it),
    written as a table of verdicts instead of a branch ladder.

    verdict of a result  | PAF tag (seconds since the channel's last chunk) | told to the chunk source
    ---------------------+--------------------------------------------------+--------------------------------
    "ended"              | Paf.ENDED                                        | stop_receiving_read
    "eject"              | Paf.EJECT (+ Paf.DELAY = the source's answer)    | unblock_read, later chunks of that read dropped
    "keep"               | Paf.KEEP                                         | stop_receiving_read
    A mapped read is ejected when depleting, an unmapped one when enriching; everything else is kept."""

    def __init__(self, unc, conf, client, pool, emit=None, clock=time.time, sim=True):
        self.unc, self.client, self.pool, self.clock = unc, client, pool, clock
        self.sim = sim      # the chunk source is the simulator: an ejection's answer is a delay, written as Paf.DELAY (scripts/uncalled:231-232)
        self.emit = emit or (lambda paf: paf.print_paf())
        self.eject_mapped = conf.realtime_mode == int(unc.RealtimePool.DEPLETE)
        self.skip_odd = conf.active_chs == int(unc.RealtimePool.EVEN)
        self.deadline = conf.duration * 3600 if conf.duration else None
        now = clock()
        self.chan = {c: _Channel(now) for c in range(1, conf.num_channels + 1)}
        self.act = {"ended": self._ended, "eject": self._eject, "keep": self._keep}

    def verdict(self, paf):
        if paf.is_ended():
            return "ended"
        return "eject" if bool(paf.is_mapped()) == self.eject_mapped else "keep"

    def _ended(self, ch, number, paf, waited):
        paf.set_float(self.unc.Paf.ENDED, waited)
        self.client.stop_receiving_read(ch, number)

    def _keep(self, ch, number, paf, waited):
        paf.set_float(self.unc.Paf.KEEP, waited)
        self.client.stop_receiving_read(ch, number)

    def _eject(self, ch, number, paf, waited):
        paf.set_float(self.unc.Paf.EJECT, waited)
        answer = self.client.unblock_read(ch, number)
        if self.sim:
            paf.set_int(self.unc.Paf.DELAY, answer)
        self.chan[ch].ejected_read = number

    def decide(self):
        """every result the pool has ready -> verdict -> PAF line"""
        for ch, number, paf in self.pool.update():
            self.act[self.verdict(paf)](ch, number, paf, self.clock() - self.chan[ch].last_chunk_at)
            self.emit(paf)

    def feed(self):
        """the source's new chunks -> the pool (channels that are switched off and ejected reads aside)"""
        for ch, chunk in self.client.get_read_chunks():
            if self.skip_odd and ch % 2:
                self.client.stop_receiving_read(ch, chunk.number)
            elif self.chan[ch].ejected_read == chunk.number:
                # (the reference's own words, spelling included: the line is part of the PAF stream its consumers see, scripts/uncalled:250)
                sys.stdout.write("# recieved chunk from %s after unblocking\n" % chunk.id)
            else:
                self.chan[ch].last_chunk_at = self.clock()
                self.pool.add_chunk(chunk)

    def run(self, sleep=time.sleep):
        """decide / feed in ticks of MAX_SLEEP until the source has stopped and nothing is left in the pool, or the
        run's duration is over"""
        while self.client.is_running or not self.pool.all_finished():
            tick = self.clock()
            self.decide()
            if not self.client.is_running:
                return          # the source ran dry: what is still undecided stays so
            self.feed()
            if self.deadline is not None and self.client.get_runtime() >= self.deadline:
                return
            spare = MAX_SLEEP - (self.clock() - tick)
            if spare > 0:
                sleep(spare)


def realtime_loop(unc, conf, client, pool, sim=True, emit=None, sleep=time.sleep):
    """`uncalled sim`'s main loop: a RealtimeSession run to its end.  `sim`: the chunk source is the simulator (the MinKNOW client,
    the only other one, is out of scope): its answer to an ejection is written as Paf.DELAY, as scripts/uncalled:231-232 does."""
    RealtimeSession(unc, conf, client, pool, emit=emit, sim=sim).run(sleep=sleep)


def sim_cmd(args):
    """`uncalled sim`: the realtime loop fed from fast5 files instead of MinKNOW (scripts/uncalled:170-256)."""
    from . import _uncalled_amd as unc
    conf = unc.Conf()
    for k, v in vars(args).items():
        if v is not None and not k.startswith("_") and hasattr(conf, k) and k not in ("realtime_mode", "active_chs"):
            setattr(conf, k, v)
    conf.realtime_mode = int(unc.RealtimePool.ENRICH if args.enrich else unc.RealtimePool.DEPLETE)
    conf.active_chs = int(unc.RealtimePool.EVEN if args.even else unc.RealtimePool.ODD if args.odd else unc.RealtimePool.FULL)
    _assert_exists(conf.bwa_prefix + ".bwt")
    _assert_exists(conf.bwa_prefix + ".uncl")
    if conf.model_path:
        _assert_exists(conf.model_path)
    pool = None
    try:
        client = unc.ClientSim(conf)
        for f in load_fast5s(args.fast5s, args.recursive):
            if f is not None:
                client.add_fast5(f)
        client.load_fast5s()
        if not client.run():
            sys.exit(1)
        pool = unc.RealtimePool(conf)
        realtime_loop(unc, conf, client, pool, sim=True)
    except KeyboardInterrupt:
        sys.stderr.write("Keyboard interrupt\n")
    if pool is not None:
        pool.stop_all()


def load_dtw_queries(fname):
    """dtw_test.cpp:27-58: lines of `read_id smp_st smp_en ref_name ref_st ref_en strand`; a later line for the same read replaces
    the earlier one, as the reference's map does."""
    queries = {}
    with open(fname) as fh:
        for no, line in enumerate(fh, 1):
            f = line.split()
            if not f or f[0].startswith("#"):
                continue
            if len(f) != 7 or f[6] not in "+-":
                sys.stderr.write("Error: %s:%d: expected `read_id smp_st smp_en ref_name ref_st ref_en strand`\n" % (fname, no))
                sys.exit(1)
            queries[f[0]] = dict(smp_st=int(f[1]), smp_en=int(f[2]), ref=f[3], ref_st=int(f[4]), ref_en=int(f[5]), fwd=f[6] == "+")
    return queries


def load_paf_queries(fname):
    """The queries of `dtw --paf`: one per mapped PAF line (read id column 1, strand column 5, reference name column 6, stretch
    [column 8, column 9)); a later line for the same read replaces the earlier one.  Unmapped lines (`*` in column 6) are skipped
    silently, a line whose stretch has fewer than five bases (no k-mer) with a word on stderr.  PAF read coordinates are bases at
    bp_per_sec / sample_rate = 450 / 4000 a sample: smp_st = column 3 * 80 // 9, smp_en = column 4 * 80 / 9 rounded up (clip_paf_queries
    cuts it to the read's samples once they are known)."""
    queries = {}
    with open(fname) as fh:
        for no, line in enumerate(fh, 1):
            f = line.rstrip("\n").split("\t")
            if not f or not f[0] or f[0].startswith("#"):
                continue
            if len(f) >= 6 and f[5] == "*":
                continue
            if len(f) < 9 or f[4] not in ("+", "-"):
                sys.stderr.write("Error: %s:%d: expected a PAF line of at least nine columns\n" % (fname, no))
                sys.exit(1)
            ref_st, ref_en = int(f[7]), int(f[8])
            if ref_en - ref_st < 5:
                sys.stderr.write("Skipping %s: %s:%d: a stretch of fewer than five bases has no k-mer\n" % (f[0], fname, no))
                continue
            queries[f[0]] = dict(smp_st=int(f[2]) * 80 // 9, smp_en=-(-int(f[3]) * 80 // 9), ref=f[5], ref_st=ref_st, ref_en=ref_en,
                                 fwd=f[4] == "+")
    return queries


def clip_paf_queries(queries, reads):
    """smp_en = min(read length in samples, what the PAF's column 4 gives)"""
    for rid, samples, _ in reads:
        q = queries[rid]
        q["smp_en"] = min(len(samples), q["smp_en"])


def extend_paf_queries(queries, reads, index, slack=1.5):
    """`--adaptive`: a query becomes the read from the hit's first sample to the read's end, against a stretch that starts where the
    hit starts on its strand (the minus strand runs leftwards from the hit's end) and is ceil(samples * bp_per_sec / sample_rate *
    slack) bases long, clipped to the sequence.  The adaptive band finds where on it the read ends."""
    import math
    from . import capi
    prm = capi.default_params()
    names = index.seq_names()
    for rid, samples, _ in reads:
        q = queries[rid]
        if q["ref"] not in names:
            continue                    # (dtw_align reports it)
        q["smp_en"] = len(samples)
        n = max(5, math.ceil((len(samples) - q["smp_st"]) * float(prm.bp_per_sec) / float(prm.sample_rate) * slack))
        if q["fwd"]:
            q["ref_en"] = min(q["ref_st"] + n, index.seq_len(names.index(q["ref"])))
        else:
            q["ref_st"] = max(q["ref_en"] - n, 0)


KMER_BASES = "ACGT"


def kmer_str(k, klen=5):
    return "".join(KMER_BASES[(int(k) >> (2 * (klen - 1 - i))) & 3] for i in range(klen))


def segment_ref_pos(ref_st, ref_en, fwd, row, klen=5):
    """forward-strand position of the first base of the k-mer that is row `row` of a query over bases [ref_st, ref_en).  The minus
    strand's rows are the forward k-mers in reverse order, each reverse-complemented (kmers_revcomp, bp.hpp:82-99): row r is the
    forward k-mer (count - 1 - r), whose first forward base is its own last base."""
    n = ref_en - ref_st - (klen - 1)
    return ref_st + row if fwd else ref_st + (n - 1 - row)


SEGMENT_COLUMNS = ("ref_name", "ref_pos", "strand", "kmer", "smp_st", "smp_span", "smp_n", "n_cols", "shared", "mean", "stdv", "level", "model_mean")


def write_segments(out, q, row_first, segs, km, model_means):
    """one line per record: the k-mer as the query's strand reads it, at its forward-strand position"""
    out.write("\t".join(SEGMENT_COLUMNS) + "\n")
    for s, r in enumerate(segs):
        row = row_first + s
        out.write("%s\t%d\t%s\t%s\t%d\t%d\t%d\t%d\t%d\t%.6g\t%.6g\t%.6g\t%.6g\n" % (
            q["ref"], segment_ref_pos(q["ref_st"], q["ref_en"], q["fwd"], row), "+" if q["fwd"] else "-", kmer_str(km[row]), int(r["smp_st"]),
            int(r["smp_span"]), int(r["smp_n"]), int(r["n_cols"]), int(r["shared"]), float(r["mean"]), float(r["stdv"]), float(r["level"]),
            float(model_means[km[row]])))


def dtw_align(index, prefix, reads, queries, max_events=50000, batch=2048, device=0, want_paths=False, band=0, segments=False, model=None,
              accumulate=None, pileup=None, refseq=None, adaptive=0):
    """The batches behind `dtw`: reads = [(id, int16 samples, (range, offset, digitisation))], queries as load_dtw_queries gives
    them.  Yields per read (id, ALIGN_RESULT record, seconds, k-mers, levels, path, SEGMENT records, SEG_INFO record), in the order of
    `reads`: k-mers, levels and path are None without want_paths, the last two None without segments.  The rows of every alignment
    are made on the device from the queries' coordinates (capi.align_ref_batch); `device` is the index's.  model: a capi.Model in
    place of the r9.4 template; accumulate: a capi.ModelAcc that takes every alignment's records; pileup: a capi.Pileup that takes
    them at their reference positions, made for `refseq`, the packed reference to align with (None: read here).  adaptive: the
    width of the adaptive band with an open end (capi.align_opts), in place of band."""
    import numpy as np
    from . import capi
    names = index.seq_names()
    if refseq is None:
        refseq = capi.RefSeq(index, prefix)     # the packed reference: read and uploaded once per run
    for b0 in range(0, len(reads), batch):
        part = reads[b0:b0 + batch]
        raw = np.concatenate([np.asarray(r[1], np.int16) for r in part]) if part else np.zeros(0, np.int16)
        offsets = np.cumsum([0] + [len(r[1]) for r in part]).astype(np.uint64)
        calib = capi.make_calib(len(part), 0, 0, 1)
        qs, stretches = [], []
        for i, (rid, _, cal) in enumerate(part):
            calib[i] = cal
            q = queries[rid]
            if q["ref"] not in names:
                sys.stderr.write("Error: no sequence '%s' in the index\n" % q["ref"])
                sys.exit(1)
            qs.append((i, q["smp_st"], q["smp_en"]))
            stretches.append((names.index(q["ref"]), q["ref_st"], q["ref_en"], q["fwd"]))
        t0 = time.time()
        out = capi.align_ref_batch(refseq, raw, offsets, calib, qs, stretches, opts=capi.align_opts(max_events=max_events, band=band, adaptive=adaptive),
                                   levels=want_paths, paths=want_paths, kmers=want_paths, segments=segments, model=model,
                                   accumulate=accumulate, pileup=pileup)
        sec = (time.time() - t0) / max(1, len(part))
        none = [None] * len(part)
        out = list(out) if isinstance(out, tuple) else [out]         # results, then what was asked for, in this order
        res = out.pop(0)
        levs, paths, kms = (out.pop(0), out.pop(0), out.pop(0)) if want_paths else (none, none, none)
        segs, infos = (out.pop(0), out.pop(0)) if segments else (none, none)
        for i, (rid, _, _) in enumerate(part):
            yield rid, res[i], sec, kms[i], levs[i], paths[i], segs[i], infos[i]


def load_query_reads(unc, fast5, queries):
    """the reads a query file names, from one fast5 file -> [(id, int16 samples, (range, offset, digitisation))]"""
    reader = unc.Fast5Reader("", "", 0, max(100, len(queries)))
    reader.add_fast5(os.path.abspath(fast5))
    for rid in queries:
        reader.add_read(rid)            # only the named reads are taken from the file (Fast5Reader::add_read)
    reads = []
    while not reader.empty():
        r = reader.pop_read()
        if r.id in queries:
            reads.append((r.id, r.raw_i16, r.calibration))
    return reads


def train_model(index, prefix, reads, queries, start=None, iters=1, min_obs=2, keep_shared=False, band=0, max_events=50000, batch=2048,
                device=0, report=None, adaptive=0):
    """The iterations behind `train`: every query aligned with the current model (dtw_align, the accumulator on the device, no
    segment outputs), then the accumulator finished into the next model with the current one as the prior.  -> the last model.
    report(iteration, records used, records dropped, k-mers kept from the prior, largest change of a mean)"""
    import numpy as np
    from . import capi
    model = start if start is not None else capi.Model.default()
    acc = capi.ModelAcc(device=device, keep_shared=keep_shared)
    for it in range(iters):
        acc.reset()
        for _ in dtw_align(index, prefix, reads, queries, max_events=max_events, batch=batch, device=device, band=band, model=model,
                           accumulate=acc, adaptive=adaptive):
            pass
        n, _, _, _, dropped = acc.read()
        nxt, kept = acc.finish(model, min_obs)
        if report:
            report(it + 1, int(n.sum()), int(dropped), kept, float(np.abs(nxt.pairs()[:, 0] - model.pairs()[:, 0]).max()))
        model = nxt
    return model


def train_cmd(args):
    """`train`: a pore model from the alignments of mapped reads, the statistics summed on the GPU"""
    from . import capi
    from . import _uncalled_amd as unc
    for f in (args.index_prefix + ".bwt", args.index_prefix + ".pac", args.fast5, args.paf) + ((args.model,) if args.model else ()):
        _assert_exists(f)
    queries = load_paf_queries(args.paf)
    reads = load_query_reads(unc, args.fast5, queries)
    clip_paf_queries(queries, reads)
    index = capi.Index(args.index_prefix, device=args.device)
    if _adaptive(args):
        extend_paf_queries(queries, reads, index, args.slack)

    def report(it, used, dropped, kept, change):
        sys.stderr.write("iteration %d: %d records used, %d dropped, %d k-mers kept from the prior, largest mean change %.6g\n" % (
            it, used, dropped, kept, change))

    model = train_model(index, args.index_prefix, reads, queries, capi.Model.load(args.model) if args.model else None, args.iters,
                        args.min_obs, args.keep_shared, args.band, args.max_events, args.batch_queries, args.device, report, args.adaptive)
    model.save(args.out)


def _adaptive(args):
    """--adaptive B as given: 0, or a width the library takes; it excludes --band"""
    if args.adaptive and (args.adaptive not in (64, 128, 256) or args.band):
        sys.stderr.write("Error: --adaptive takes 64, 128 or 256 and goes without --band\n")
        sys.exit(1)
    return args.adaptive


PILEUP_COLUMNS = ("contig", "pos", "strand", "kmer", "cov", "mean", "stdv", "dwell", "model_mean", "model_stdv", "z")
PILEUP_CONTROL_COLUMNS = ("ctl_cov", "ctl_mean", "ctl_stdv", "t")
PILEUP_KS_COLUMNS = ("ks_d", "ks", "ks_bucket")


def parse_region(text, names, index):
    """NAME:ST-EN -> (rid, st, en); the name may hold colons itself, so the last one counts"""
    name, _, span = text.rpartition(":")
    st, _, en = span.partition("-")
    if name not in names or not st.isdigit() or not en.isdigit() or int(st) > int(en) or int(en) > index.seq_len(names.index(name)):
        sys.stderr.write("Error: --region %s: expected NAME:ST-EN inside a sequence of the index\n" % text)
        sys.exit(1)
    return names.index(name), int(st), int(en)


def pileup_fill(unc, index, prefix, refseq, pileup, fast5, paf, model, args):
    """every mapped line of `paf` aligned as `dtw --paf` aligns it, the records piled up on the device -> alignments made"""
    from . import capi
    queries = load_paf_queries(paf)
    reads = load_query_reads(unc, fast5, queries)
    clip_paf_queries(queries, reads)
    if _adaptive(args):
        extend_paf_queries(queries, reads, index, args.slack)
    done = 0
    for _, r, _, _, _, _, _, _ in dtw_align(index, prefix, reads, queries, max_events=args.max_events, batch=args.batch_queries,
                                            device=args.device, band=args.band, model=model, pileup=pileup, refseq=refseq,
                                            adaptive=args.adaptive):
        done += int(r["status"]) in (capi.DTW_OK, capi.DTW_REF_END)
    return done


def write_pileup(out, names, pileup, control, min_cov, model, ks=False):
    """one line per covered bin, by bin index; floats as %.17g, which names a double exactly.  ks: both pile-ups carry histograms, and
    three columns more give their Kolmogorov-Smirnov distance (every covered bin holds min_cov >= 1 records in both)"""
    out.write("\t".join(PILEUP_COLUMNS + (PILEUP_CONTROL_COLUMNS if control is not None else ()) + (PILEUP_KS_COLUMNS if ks else ())) + "\n")
    bins = pileup.covered(min_cov, other=control)
    rid, pos, fwd = pileup.locate(bins)
    st = pileup.stats(bins, model)
    cs = control.stats(bins, model) if control is not None else None
    t = {}
    if control is not None:       # Welch's t needs two records on either side
        both = [i for i in range(len(bins)) if st["n"][i] >= 2 and cs["n"][i] >= 2]
        t = dict(zip(both, pileup.compare(control, bins[both])["t"])) if both else {}
    kd = pileup.ks(control, bins) if ks else None
    for i in range(len(bins)):
        line = "%s\t%d\t%s\t%s\t%d\t%.17g\t%.17g\t%.17g\t%.17g\t%.17g\t%.17g" % (
            names[int(rid[i])], int(pos[i]), "+" if fwd[i] else "-", kmer_str(st["kmer"][i]), int(st["n"][i]), st["mean"][i], st["sd"][i],
            st["dwell"][i], st["model_mean"][i], st["model_stdv"][i], st["z"][i])
        if control is not None:
            line += "\t%d\t%.17g\t%.17g\t%.17g" % (int(cs["n"][i]), cs["mean"][i], cs["sd"][i], t.get(i, float("nan")))
        if ks:
            line += "\t%.17g\t%.17g\t%d" % (kd["d"][i], kd["ks"][i], int(kd["bucket"][i]))
        out.write(line + "\n")
    return len(bins)


def pileup_cmd(args):
    """`pileup`: the signal of many alignments per reference position and strand, summed on the GPU, against the model's expectation
    and optionally against a control sample's"""
    from . import capi
    from . import _uncalled_amd as unc
    inputs = [args.fast5, args.paf] + (list(args.control) if args.control else [])
    for f in [args.index_prefix + ".bwt", args.index_prefix + ".pac"] + inputs + ([args.model] if args.model else []):
        _assert_exists(f)
    min_cov = args.min_cov if args.min_cov is not None else (2 if args.control else 1)
    if min_cov < 1:
        sys.stderr.write("Error: --min-cov must be at least 1\n")
        sys.exit(1)
    if args.ks and not args.control:
        sys.stderr.write("Error: --ks compares two samples: it needs --control\n")
        sys.exit(1)
    index = capi.Index(args.index_prefix, device=args.device)
    names = index.seq_names()
    regions = [parse_region(r, names, index) for r in args.region] if args.region else None
    refseq = capi.RefSeq(index, args.index_prefix)
    model = capi.Model.load(args.model) if args.model else None
    pileup = capi.Pileup(refseq, regions, args.keep_shared)
    control = capi.Pileup(refseq, regions, args.keep_shared) if args.control else None
    for pu, (fast5, paf), what in ((pileup, (args.fast5, args.paf), "sample"), (control, args.control or (None, None), "control")):
        if pu is None:
            continue
        if args.ks:
            pu.enable_hist(args.ks_width, model)
        done = pileup_fill(unc, index, args.index_prefix, refseq, pu, fast5, paf, model, args)
        sys.stderr.write("%s: %d alignments, %d records added, %d dropped, %d outside the regions\n" % (
            (what, done) + tuple(pu.counters()[i] for i in (2, 0, 1))))
    with open(args.out, "w") as out:
        n = write_pileup(out, names, pileup, control, min_cov, model, args.ks)
    sys.stderr.write("%d bins with at least %d records written to %s\n" % (n, min_cov, args.out))


def dtw_cmd(args):
    """`dtw_test` (src/dtw_test.cpp:62-176): one signal-to-reference alignment per query line, all of them on the GPU in batches."""
    from . import capi
    from . import _uncalled_amd as unc
    _assert_exists(args.index_prefix + ".bwt")
    _assert_exists(args.index_prefix + ".pac")
    _assert_exists(args.fast5)
    _assert_exists(args.queries)
    if args.segments and args.out_prefix is None:
        sys.stderr.write("Error: --segments needs -o\n")
        sys.exit(1)
    if args.model:
        _assert_exists(args.model)
    queries = load_paf_queries(args.queries) if args.paf else load_dtw_queries(args.queries)
    reads = load_query_reads(unc, args.fast5, queries)
    if args.paf:
        clip_paf_queries(queries, reads)
    index = capi.Index(args.index_prefix, device=args.device)
    if _adaptive(args):
        if not args.paf:
            sys.stderr.write("Error: --adaptive needs --paf\n")
            sys.exit(1)
        extend_paf_queries(queries, reads, index, args.slack)
    model = capi.Model.load(args.model) if args.model else None
    for rid, r, sec, km, lev, path, segs, seg_info in dtw_align(index, args.index_prefix, reads, queries, max_events=args.max_events,
                                                      batch=args.batch_queries, device=args.device, want_paths=args.out_prefix is not None,
                                                      band=args.band, segments=args.segments, model=model, adaptive=args.adaptive):
        st = int(r["status"])
        if st == capi.ALIGN_TOO_MANY:
            sys.stderr.write("Skipping %s\n" % rid)            # dtw_test.cpp:156-159
            continue
        if st == capi.DTW_BAND_TOO_NARROW:
            sys.stdout.write("%s\t%.6g\t%.6g\tstatus %d\n" % (rid, 0.0, sec, st))      # (nothing computed: the line says why)
            sys.stdout.flush()
            continue
        if st not in (capi.DTW_OK, capi.DTW_LEFT_BAND, capi.DTW_REF_END):
            sys.stderr.write("Skipping %s: %s\n" % (rid, "no events left to align" if st == capi.ALIGN_NO_COLUMNS else "status %d" % st))
            continue
        if args.out_prefix is not None:
            means = model.tables(False)[0] if model is not None else capi.dtw_model_tables()[0]
            with open(args.out_prefix + rid + ".txt", "w") as out:
                for j, i in path[::-1]:                          # from the start of the alignment to its end
                    out.write("%d\t%d\t%s\t%.6g\t%.6g\n" % (j, i, kmer_str(km[i]), lev[j], abs(float(lev[j]) - float(means[km[i]]))))
            if args.segments and st in (capi.DTW_OK, capi.DTW_REF_END):      # (a path that left the band has no start: no records)
                with open(args.out_prefix + rid + ".segments.tsv", "w") as out:
                    write_segments(out, queries[rid], int(seg_info["row_first"]), segs, km, means)
        sys.stdout.write("%s\t%.6g\t%.6g%s\n" % (rid, float(r["dtw"]["mean_score"]), sec, "\tstatus %d" % st if st else ""))
        sys.stdout.flush()


def get_parser():
    from . import index_params, pafstats
    d = index_params.DEFAULTS
    ap = argparse.ArgumentParser(prog="uncalled_amd", description="Rapidly maps raw nanopore signal to DNA references (MI355X)")
    sp = ap.add_subparsers(dest="subcmd")
    sp.required = True

    p = sp.add_parser("index", help="Builds the UNCALLED index of a FASTA reference")
    p.add_argument("fasta_filename", type=str, help="FASTA file to index")
    p.add_argument("-o", "--bwa-prefix", type=str, default=None, help="Index output prefix. Will use input fasta filename by default")
    p.add_argument("-s", "--max-sample-dist", type=int, default=d["max_sample_dist"], help="Maximum average sampling distance between reference self-alignments.")
    p.add_argument("--min-samples", type=int, default=d["min_samples"], help="Minimum number of self-alignments to produce (approximate, due to deterministically random start locations)")
    p.add_argument("--max-samples", type=int, default=d["max_samples"], help="Maximum number of self-alignments to produce (approximate, due to deterministically random start locations)")
    p.add_argument("-k", "--kmer-len", type=int, default=d["kmer_len"], help="Model k-mer length")
    p.add_argument("-1", "--matchpr1", type=float, default=d["matchpr1"], help="Minimum event match probability")
    p.add_argument("-2", "--matchpr2", type=float, default=d["matchpr2"], help="Maximum event match probability")
    p.add_argument("-f", "--pathlen-percentile", type=float, default=d["pathlen_percentile"], help="")
    p.add_argument("-m", "--max-replen", type=int, default=d["max_replen"], help="")
    p.add_argument("--probs", type=str, default=None, help="Find parameters with specified target probabilites (comma separated)")
    p.add_argument("--speeds", type=str, default=None, help="Find parameters with specified speed coefficents (comma separated)")
    p.add_argument("--device", type=int, default=0, help="GPU ordinal")

    p = sp.add_parser("map", help="Map fast5 files to a DNA reference")
    p.add_argument("bwa_prefix", type=str, help="BWA prefix to mapping to. Must be processed by \"uncalled index\".")
    p.add_argument("-p", "--idx-preset", type=str, default="default", help="Mapping mode")
    p.add_argument("fast5s", nargs="+", type=str, help="Reads to map: directories, fast5 files, or text files with one fast5 name per line")
    p.add_argument("-r", "--recursive", action="store_true")
    p.add_argument("-l", "--read-list", type=str, default=None, help="Only map reads with these ids")
    p.add_argument("-n", "--max-reads", type=int, default=None, help="Maximum number of reads to map")
    p.add_argument("-t", "--threads", type=int, default=1, help="1 (default): the reads are mapped exactly as `uncalled map -t 1` maps them, in input order (the few reads whose predecessor left Mapper state behind are mapped twice); "
                        "N > 1: every read independently, which is what the reference's N threads give up to their scheduling. No host threads are created either way: reads are batched onto the GPU")
    p.add_argument("--num-channels", type=int, default=512)
    p.add_argument("-e", "--max-events", type=int, default=30000, help="Will give up on a read after this many events have been processed")
    p.add_argument("-c", "--max-chunks", type=int, default=1000000, help="Will give up on a read after this many chunks have been processed")
    p.add_argument("--chunk-time", type=float, default=1, help="Length of chunks in seconds")
    p.add_argument("--device", type=int, default=0, help="GPU ordinal")
    p.add_argument("--model", dest="model_path", type=str, default=None, help="Pore model file (a header line, then `kmer level_mean level_stdv` "
                   "for all 1024 5-mers) to map with in place of the built-in r9.4 template")
    p.add_argument("--batch-reads", type=int, default=None, help="Reads per GPU batch (default: four times what the mapper keeps in flight; the first batch is one load)")
    p.add_argument("--gpus", type=int, default=1, help="GPUs of this node to use: one worker process each, fast5 files dealt round-robin")

    p = sp.add_parser("sim", help="Simulate real-time targeted sequencing from fast5 files (enrich / deplete decisions per read)")
    p.add_argument("bwa_prefix", type=str, help="BWA prefix to mapping to. Must be processed by \"uncalled index\".")
    p.add_argument("-p", "--idx-preset", type=str, default="default", help="Mapping mode")
    p.add_argument("fast5s", nargs="+", type=str, help="Reads to replay: directories, fast5 files, or text files with one fast5 name per line")
    p.add_argument("-r", "--recursive", action="store_true")
    mode = p.add_mutually_exclusive_group(required=True)
    mode.add_argument("-D", "--deplete", action="store_true", help="Will eject reads that align to the reference")
    mode.add_argument("-E", "--enrich", action="store_true", help="Will eject reads that do not align to the reference")
    chs = p.add_mutually_exclusive_group()
    chs.add_argument("--even", action="store_true", help="Will only eject reads from even channels")
    chs.add_argument("--odd", action="store_true", help="Will only eject reads from odd channels")
    p.add_argument("-l", "--read-list", type=str, default=None, help="Only replay reads with these ids")
    p.add_argument("-n", "--max-reads", type=int, default=None, help="Maximum number of reads to replay")
    p.add_argument("--num-channels", type=int, default=512)
    p.add_argument("-e", "--max-events", type=int, default=30000)
    p.add_argument("-c", "--max-chunks", type=int, default=10, help="Will give up on a read after this many chunks have been processed")
    p.add_argument("--chunk-time", type=float, default=1, help="Length of chunks in seconds")
    p.add_argument("--model", dest="model_path", type=str, default=None, help="Pore model file (a header line, then `kmer level_mean level_stdv` "
                   "for all 1024 5-mers) to map with in place of the built-in r9.4 template")
    p.add_argument("--duration", type=float, default=None, help="Duration to map real-time run in hours")
    p.add_argument("--device", type=int, default=0, help="GPU ordinal")

    p = sp.add_parser("dtw", help="Align reads' signal to stretches of the reference by dynamic time warping (the reference's dtw_test)",
                      description="One alignment per query line `read_id smp_st smp_en ref_name ref_st ref_en strand` (smp_en 0: to the "
                      "read's end): events of the sample range, stalls masked, normalised to the levels of the stretch's k-mers, DTWr94d. "
                      "Prints `read_id  mean_score  seconds` per read (seconds: the batch's wall time over its queries). -o writes one "
                      "path file per read, from the start of the alignment to its end: event index, k-mer index, k-mer, level, cost. "
                      "(The reference's print_path indexes the k-mers with the event index and the events with the k-mer index and can "
                      "read past both; that is not reproduced.)")
    p.add_argument("index_prefix", type=str, help="BWA prefix of the reference (needs the .pac)")
    p.add_argument("fast5", type=str, help="fast5 file that holds the reads")
    p.add_argument("queries", type=str, help="Query file, one line per read (with --paf: a PAF file)")
    p.add_argument("--paf", action="store_true", help="QUERIES is a PAF file, such as `map` writes: one alignment per mapped line, of the read in "
                   "column 1 on the strand of column 5 against bases [column 8, column 9) of the sequence named in column 6. The sample range "
                   "comes from the read coordinates, which are bases at 450 / 4000 a sample: smp_st = column 3 * 80 // 9, smp_en = column 4 * 80 / 9 "
                   "rounded up, at most the read's samples. Unmapped lines (`*` in column 6) are skipped silently, a line whose stretch has "
                   "fewer than five bases is reported on stderr and skipped; of several lines for one read the last one counts. May be "
                   "combined with --band or not")
    p.add_argument("-o", "--out-prefix", type=str, default=None, help="Write the path of read ID to OUT_PREFIX + ID + .txt")
    p.add_argument("--segments", action="store_true", help="With -o: also write OUT_PREFIX + ID + .segments.tsv, the alignment in the read's "
                   "sample coordinates, one line per reference k-mer on the path: ref_name, ref_pos (forward-strand position of the k-mer's "
                   "first base), strand, kmer, smp_st (first sample), smp_span (samples to the end of its last event), smp_n (samples of its "
                   "events), n_cols (events), shared (1: its first event is also the previous k-mer's last), mean, stdv (pA over its samples), "
                   "level (mean, normalised), model_mean")
    p.add_argument("--max-events", type=int, default=50000, help="Skip reads with more events than this (the reference's 50000; 0: no limit -- "
                   "2 bits per cell make alignments affordable here that the reference skips)")
    p.add_argument("--band", type=int, default=0, help="Align within a band of this half-width (in k-mers) around the diagonal: work and memory "
                   "grow with the events times the band, not with events times k-mers (0: the full matrix). A line then ends in "
                   "`status 5` (the band is too narrow to reach the end: not aligned) or `status 6` (the path left the band) where so")
    p.add_argument("--adaptive", type=int, default=0, metavar="B", help="With --paf: align the whole read from where its hit starts. The query is the read from the hit's first sample to its end, the stretch starts at the hit's start on its strand and is ceil(samples * bp_per_sec / sample_rate * F) bases long (--slack F), and the DTW runs in a band of B k-mers (64, 128 or 256) that follows the path, with an open end. A line then ends in `status 7` where the alignment ends in the stretch's last k-mer (the stretch was too short) or `status 6` where the path left the band")
    p.add_argument("--slack", type=float, default=1.5, metavar="F", help="With --adaptive: the stretch is F times the bases the samples are expected to cover")
    p.add_argument("--batch-queries", type=int, default=2048, help="Queries per GPU batch")
    p.add_argument("--device", type=int, default=0, help="GPU ordinal")

    p.add_argument("--model", type=str, default=None, help="Pore model file to align with in place of the built-in r9.4 template")

    p = sp.add_parser("train", help="Train a pore model from the alignments of mapped reads",
                      description="Every mapped line of PAF is aligned as `dtw --paf` aligns it, with the current model; the normalised level "
                      "of every reference k-mer on every path is summed per k-mer on the GPU (fixed point: the result does not depend on the "
                      "order or the batching), and the means and deviations become the next model. A k-mer with fewer than MIN_OBS records "
                      "keeps its row of the model before. One line per iteration goes to stderr.")
    p.add_argument("index_prefix", type=str, help="BWA prefix of the reference (needs the .pac)")
    p.add_argument("fast5", type=str, help="fast5 file that holds the reads")
    p.add_argument("paf", type=str, help="PAF file, such as `map` writes")
    p.add_argument("-o", "--out", type=str, required=True, help="The model file to write")
    p.add_argument("--model", type=str, default=None, help="Model file to start from (default: the built-in r9.4 template)")
    p.add_argument("--iters", type=int, default=1, help="Iterations of align and re-estimate")
    p.add_argument("--min-obs", type=int, default=10, help="Records a k-mer needs for a row of its own (at least 2)")
    p.add_argument("--keep-shared", action="store_true", help="Also count a k-mer whose first event is the previous k-mer's last")
    p.add_argument("--band", type=int, default=0, help="As in dtw")
    p.add_argument("--adaptive", type=int, default=0, metavar="B", help="As in dtw: whole reads, aligned from where their hits start")
    p.add_argument("--slack", type=float, default=1.5, metavar="F", help="With --adaptive: the stretch is F times the bases the samples are expected to cover")
    p.add_argument("--max-events", type=int, default=50000, help="As in dtw")
    p.add_argument("--batch-queries", type=int, default=2048, help="Queries per GPU batch")
    p.add_argument("--device", type=int, default=0, help="GPU ordinal")

    p = sp.add_parser("pileup", help="Pile the aligned signal of mapped reads up per reference position and strand",
                      description="Every mapped line of PAF is aligned as `dtw --paf` aligns it; the normalised level and the dwell of every "
                      "reference k-mer on every path are summed on the GPU per position of the k-mer's leftmost base and strand (fixed point: "
                      "the result does not depend on the order or the batching). One line per position and strand with at least MIN_COV "
                      "records: contig, pos, strand, kmer, cov, mean, stdv, dwell (samples), the model's mean and stdv for the k-mer, and "
                      "z = (mean - model_mean) / model_stdv * sqrt(cov). With --control: positions covered in both samples, the control's "
                      "cov, mean, stdv, and Welch's t of the two means (nan where either sample has fewer than two records there). With --ks as well: "
                      "ks_d, the two-sample Kolmogorov-Smirnov distance of the two samples' level histograms at the position (64 buckets of "
                      "KS_WIDTH levels, bucket 32 beginning at the model's mean), ks = ks_d * sqrt(cov * ctl_cov / (cov + ctl_cov)), and "
                      "ks_bucket, the bucket where the two cumulative distributions lie furthest apart. Floats are printed as %.17g.")
    p.add_argument("index_prefix", type=str, help="BWA prefix of the reference (needs the .pac)")
    p.add_argument("fast5", type=str, help="fast5 file that holds the reads")
    p.add_argument("paf", type=str, help="PAF file, such as `map` writes")
    p.add_argument("-o", "--out", type=str, required=True, help="The TSV file to write")
    p.add_argument("--control", nargs=2, metavar=("FAST5", "PAF"), default=None, help="A second sample to compare with")
    p.add_argument("--ks", action="store_true", help="With --control: level histograms for both samples (256 bytes of GPU memory more per "
                   "position and strand: use --region) and three columns ks_d, ks, ks_bucket")
    p.add_argument("--ks-width", type=float, default=0.25, metavar="W", help="Width of a histogram bucket in normalised levels (default 0.25: "
                   "the 64 buckets span the model's mean -8 .. +8; the default is a choice that nobody has measured against data)")
    p.add_argument("--region", action="append", default=None, metavar="NAME:ST-EN", help="Pile up only inside these bases of the reference "
                   "(repeatable; regions may not overlap; default: every sequence, whole -- 80 bytes of GPU memory per base)")
    p.add_argument("--min-cov", type=int, default=None, help="Records a position needs to be written (default 1, with --control 2)")
    p.add_argument("--model", type=str, default=None, help="Pore model file to align with and compare against (default: the built-in r9.4 template)")
    p.add_argument("--keep-shared", action="store_true", help="Also count a k-mer whose first event is the previous k-mer's last")
    p.add_argument("--band", type=int, default=0, help="As in dtw")
    p.add_argument("--adaptive", type=int, default=0, metavar="B", help="As in dtw: whole reads, aligned from where their hits start")
    p.add_argument("--slack", type=float, default=1.5, metavar="F", help="With --adaptive: the stretch is F times the bases the samples are expected to cover")
    p.add_argument("--max-events", type=int, default=50000, help="As in dtw")
    p.add_argument("--batch-queries", type=int, default=2048, help="Queries per GPU batch")
    p.add_argument("--device", type=int, default=0, help="GPU ordinal")

    p = sp.add_parser("mask", help="Mask repeats of a FASTA reference before indexing it (the reference's masking/ scripts, on the GPU)",
                      description="`mask internal` masks the most frequent k-mer of the reference, ITERS times over (mask_internal.sh and "
                      "mask_kmers.py); ties go to the k-mer that sorts first, and the run ends early once no k-mer occurs twice. `mask external` "
                      "masks every stretch of the target whose windows of MIN_LEN bases occur more than MIN_COPY times in an index, both strands "
                      "counted (mask_external.sh).")
    from . import mask
    mask.add_opts(p)

    p = sp.add_parser("pafstats", help="Computes speed and accuracy of UNCALLED mappings")
    pafstats.add_opts(p)
    return ap


def main(argv=None):
    args = get_parser().parse_args(argv)
    if args.subcmd == "index":
        index_cmd(args)
    elif args.subcmd == "map":
        map_cmd(args)
    elif args.subcmd == "sim":
        sim_cmd(args)
    elif args.subcmd == "dtw":
        dtw_cmd(args)
    elif args.subcmd == "train":
        train_cmd(args)
    elif args.subcmd == "pileup":
        pileup_cmd(args)
    elif args.subcmd == "mask":
        from . import mask
        mask.run(args)
    else:
        from . import pafstats
        pafstats.run(args)


if __name__ == "__main__":
    main()
