"""Throughput of the batched calls (GlobalAligner.score_pairs / score_matrix; align_pairs, 5.11): one
JSON line per workload with pairs, cells, ms (median of 5 calls after 2 warm-ups), pairs_per_s and cells_per_s.

    python tools/batch_bench.py                 B1, B2, B3
    python tools/batch_bench.py --loop K        K of B1's pairs through GlobalAligner(traceback=False).align, one at a
                                                time (only API that predates the batch calls: runs on older trees too)
    python tools/batch_bench.py --crossover     one pair per call through the batch kernel and through the single-pair
                                                fill, at growing sizes (the GA_BATCH_MAX_CELLS default)
    python tools/batch_bench.py --align         B1 and B2 through align_pairs (strings included), with the kernel, host
                                                table and host decode ms of the last call and us per pair, and the
                                                engine call's own ms (ga_batch_align: median, least and most of the
                                                timed calls) with its table and kernel parts; each with the tables
                                                built on 8 host threads, on one, and -- where the tree has the
                                                route -- on the device; then the device generator alone on one item
                                                of growing length (--align-host: without the device route, for older
                                                trees)
    python tools/batch_bench.py --align-loop K  K of B1's pairs through random.seed(s) + GlobalAligner.align, one at a
                                                time (runs on older trees too)
    python tools/batch_bench.py --align-crossover   one pair per align_pairs call through the batch kernel and through
                                                the single-pair path, at growing sizes (GA_BATCH_ALIGN_MAX_CELLS)
    python tools/batch_bench.py --sample        S1, S2, S3 through sample_alignments, each beside what
                                                the tree could do for the same request before that call existed --
                                                align_pairs on the repeated lists with the same seeds (S1, S2), a loop
                                                of random.seed(s) + align over 32 of the seeds (S3) --, in alternating
                                                rounds of one process: median, least and most of 5 after 2 warm-ups,
                                                with the engine's own parts of the last call
    python tools/batch_bench.py --count         B1 and S3's 10k x 10k pair through count_alignments:
                                                median, least and most of 5 after 2 warm-ups, with the count launch's
                                                kernel ms beside the fill's for the same batch (medians over the timed
                                                calls of the same run), the count's ns per cell, and the counts' range
    python tools/batch_bench.py --rank          B1 with 16 ranks a pair and S3's 10k x 10k pair with 64 ranks through
                                                alignments_by_rank, the ranks drawn below the counts a
                                                first call returns: median, least and most of 5 after 2 warm-ups, with
                                                the table and walk launches' kernel ms, and count_alignments's count
                                                launch on the same batch in the same run; B1 once more with the tables'
                                                cap raised so that it takes one chunk
    python tools/batch_bench.py --support       B1 cut to the pairs whose dense output fits one chunk's default cap, and
                                                S3's 10k x 10k pair, through match_support: median,
                                                least and most of 5 after 2 warm-ups, with the N-table, flow and gather
                                                launches' kernel ms and count_alignments's count launch on the same
                                                batch in the same run

Workloads (SplitMix64 sequences of tests.conftest, lengths from a seeded random.Random):
  B1  4096 DNA pairs, lengths 200-400         B2  1024 BLOSUM62 pairs, lengths 100-600
  B3  score_matrix of 256 DNA sequences of about 300
  S1  256 of B1's pairs x 16 samples          S2  one 300 x 257 DNA pair (random.Random(5)) x 4096 samples
  S3  one 10k x 10k DNA pair x 256 samples (the single-pair fill's words, walked by batch_walks_kernel)"""
import argparse
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from globalign_amd import GlobalAligner, _native  # noqa: E402
from tests.conftest import splitmix_seq  # noqa: E402

DNA = dict(match_score=2, mismatch_score=-3, gap_open_score=-5, gap_extension_score=-1)
BLOSUM = dict(scoring_mat_name="BLOSUM62", gap_open_score=-10)
WARMUP, REPEATS = 2, 5


def pairs_of(count, lo, hi, alphabet, seed):
    rng = random.Random(seed)
    return [(splitmix_seq(rng.randint(lo, hi), 2 * k + 1, alphabet), splitmix_seq(rng.randint(lo, hi), 2 * k + 2, alphabet))
            for k in range(count)]


def timed(call):
    for _ in range(WARMUP):
        call()
    ms = []
    for _ in range(REPEATS):
        t0 = time.perf_counter()
        call()
        ms.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ms)


def report(name, pairs, cells, ms, **extra):
    print(json.dumps(dict(workload=name, pairs=pairs, cells=cells, ms=round(ms, 4), pairs_per_s=round(pairs / ms * 1e3, 1),
                          cells_per_s=round(cells / ms * 1e3, 1), **extra)), flush=True)


def workloads():
    b1 = pairs_of(4096, 200, 400, "dna", 1)
    al = GlobalAligner(max_seq_len_prod=None, **DNA)
    a, b = [p[0] for p in b1], [p[1] for p in b1]
    report("B1", len(b1), sum(len(x) * len(y) for x, y in b1), timed(lambda: al.score_pairs(a, b)),
           kernel_ms=round(_native.default_engine(0).kernel_ms()[0], 4))
    b2 = pairs_of(1024, 100, 600, "protein", 2)
    al2 = GlobalAligner(max_seq_len_prod=None, **BLOSUM)
    a2, b2s = [p[0] for p in b2], [p[1] for p in b2]
    report("B2", len(b2), sum(len(x) * len(y) for x, y in b2), timed(lambda: al2.score_pairs(a2, b2s)),
           kernel_ms=round(_native.default_engine(0).kernel_ms()[0], 4))
    rng = random.Random(3)
    seqs = [splitmix_seq(rng.randint(280, 320), 1000 + k, "dna") for k in range(256)]
    total = sum(len(s) for s in seqs)
    report("B3", len(seqs) ** 2, total * total, timed(lambda: al.score_matrix(seqs)),
           kernel_ms=round(_native.default_engine(0).kernel_ms()[0], 4))


def loop(count):
    """The per-pair loop a user writes without the batch calls: one align per pair."""
    b1 = pairs_of(count, 200, 400, "dna", 1)  # a prefix of B1 (the same seeds and lengths)
    al = GlobalAligner(max_seq_len_prod=None, traceback=False, **DNA)

    def call():
        for x, y in b1:
            al.align(x, y)

    report("B1-loop", len(b1), sum(len(x) * len(y) for x, y in b1), timed(call))


def crossover():
    for side in (256, 512, 768, 1024, 1536, 2048, 3072, 4096):
        x, y = splitmix_seq(side, 1, "dna"), splitmix_seq(side, 2, "dna")
        for route, limit in (("kernel", 1 << 40), ("single", 0)):
            _native.OPTIONS["GA_BATCH_MAX_CELLS"] = str(limit)
            al = GlobalAligner(max_seq_len_prod=None, **DNA)
            ms = timed(lambda: al.score_pairs([x], [y]))
            report(f"1x {side}x{side} {route}", 1, side * side, ms,
                   kernel_ms=round(_native.default_engine(0).kernel_ms()[0], 4))
        del _native.OPTIONS["GA_BATCH_MAX_CELLS"]


def align_workloads(device):
    def run(name, pairs, kw, tables="host", **options):
        _native.OPTIONS.update({k: str(v) for k, v in options.items()})
        try:
            al = GlobalAligner(max_seq_len_prod=None, **kw)
            a, b = [p[0] for p in pairs], [p[1] for p in pairs]
            route = {} if tables == "host" else {"tables": tables}  # (older trees have no such argument)
            parts = []

            def call():
                al.align_pairs(a, b, seeds=1, **route)
                parts.append(_native.default_engine(0).batch_align_timings())

            ms = timed(call)
            t, parts = parts[-1], parts[-REPEATS:]
            engine = {f"engine_{k}": round(statistics.median(x[k] for x in parts), 4) for k in ("call_ms", "table_ms", "kernel_ms")}
            calls = [x["call_ms"] for x in parts]
            report(name, len(pairs), sum(len(x) * len(y) for x, y in pairs), ms, us_per_pair=round(ms * 1e3 / len(pairs), 3),
                   **{k: round(v, 4) for k, v in t.items()}, **engine, engine_call_ms_min=round(min(calls), 4),
                   engine_call_ms_max=round(max(calls), 4), tables=tables, **options)
        finally:
            for k in options:
                del _native.OPTIONS[k]

    for name, pairs, kw in (("B1-align", pairs_of(4096, 200, 400, "dna", 1), DNA),
                            ("B2-align", pairs_of(1024, 100, 600, "protein", 2), BLOSUM)):
        run(name, pairs, kw, GA_BATCH_RNG_THREADS=8)
        run(name, pairs, kw, GA_BATCH_RNG_THREADS=1)
        if device:
            run(name, pairs, kw, tables="device")
    if device:
        generator_sweep()


def generator_sweep():
    """batch_rng_kernel alone on ONE item of growing length, through the debug entry: its event time (a lone wave:
    what the longest device-routed item of a launch costs) beside one host thread's time for the same table."""
    _native.OPTIONS["GA_BATCH_RNG_DEVICE_MAX_STEPS"] = str(1 << 20)
    try:
        eng = _native.default_engine(0)
        for steps in (256, 512, 1024, 2048, 4096, 8192, 16384, 32768, 65536):
            gen, host = [], []
            for k in range(WARMUP + REPEATS):
                _, _, status = eng.debug_pair_tables([k + 1], [steps], rng_tables="device")
                assert not status.any()
                gen.append(eng.batch_align_timings()["table_ms"])
                t0 = time.perf_counter()
                eng.debug_pair_tables([k + 1], [steps], rng_tables="host")
                host.append((time.perf_counter() - t0) * 1e3)
            gen, host = gen[WARMUP:], host[WARMUP:]
            print(json.dumps(dict(workload="generator-1-item", steps=steps, generator_ms=round(statistics.median(gen), 4),
                                  generator_ms_min=round(min(gen), 4), generator_ms_max=round(max(gen), 4),
                                  generator_ns_per_step=round(statistics.median(gen) * 1e6 / steps, 1),
                                  host_thread_ms=round(statistics.median(host), 4))), flush=True)
    finally:
        del _native.OPTIONS["GA_BATCH_RNG_DEVICE_MAX_STEPS"]


def align_loop(count):
    """The per-pair loop a user writes without align_pairs: random.seed + one align per pair."""
    b1 = pairs_of(count, 200, 400, "dna", 1)
    al = GlobalAligner(max_seq_len_prod=None, **DNA)

    def call():
        for k, (x, y) in enumerate(b1):
            random.seed(1 + k)
            al.align(x, y)

    ms = timed(call)
    report("B1-align-loop", len(b1), sum(len(x) * len(y) for x, y in b1), ms, us_per_pair=round(ms * 1e3 / len(b1), 3))


def align_crossover():
    for side in (64, 128, 256, 384, 512, 768, 1024, 1536, 2048):
        x, y = splitmix_seq(side, 1, "dna"), splitmix_seq(side, 2, "dna")
        for route, limit in (("kernel", 1 << 40), ("single", 0)):
            _native.OPTIONS["GA_BATCH_ALIGN_MAX_CELLS"] = str(limit)
            al = GlobalAligner(max_seq_len_prod=None, **DNA)
            ms = timed(lambda: al.align_pairs([x], [y], seeds=1))
            t = _native.default_engine(0).batch_align_timings()
            report(f"1x {side}x{side} align {route}", 1, side * side, ms,
                   **{k: round(t[k], 4) for k in ("kernel_ms", "walk_ns_per_step", "fill_ns_per_cell")})
        del _native.OPTIONS["GA_BATCH_ALIGN_MAX_CELLS"]


def sample_workloads():
    def rounds(new, old):
        for _ in range(WARMUP):
            new(), old()
        ms = ([], [])
        for _ in range(REPEATS):
            for which, call in enumerate((new, old)):
                t0 = time.perf_counter()
                call()
                ms[which].append((time.perf_counter() - t0) * 1e3)
        return ms

    def spread(ms):
        return dict(ms=round(statistics.median(ms), 4), ms_min=round(min(ms), 4), ms_max=round(max(ms), 4))

    def run(name, pairs, count, old_samples=None):
        """pairs x count samples from seed base 1; the other side: the same request (old_samples of the samples of
        each pair, per-sample figures reported for both)."""
        al = GlobalAligner(max_seq_len_prod=None, **DNA)
        a, b = [p[0] for p in pairs], [p[1] for p in pairs]
        eng, parts = _native.default_engine(0), {}

        def new():
            al.sample_alignments(a, b, samples=count, seeds=1)
            parts["new"] = eng.batch_sample_timings()
            parts["info"] = eng.batch_sample_info()

        if old_samples is None:
            flat_a = [x for x in a for _ in range(count)]
            flat_b = [x for x in b for _ in range(count)]
            n_old = len(flat_a)

            def old():
                al.align_pairs(flat_a, flat_b, seeds=1)
                parts["old"] = eng.batch_align_timings()
        else:
            n_old = len(pairs) * old_samples

            def old():
                for k in range(len(pairs)):
                    for t in range(old_samples):
                        random.seed(1 + k * count + t)
                        al.align(a[k], b[k])

        ms_new, ms_old = rounds(new, old)
        n_new = len(pairs) * count
        print(json.dumps(dict(workload=name, pairs=len(pairs), samples=n_new, cells=sum(len(x) * len(y) for x, y in pairs),
                              sample_alignments=dict(spread(ms_new), us_per_sample=round(statistics.median(ms_new) / n_new * 1e3, 3),
                                                     **{k: round(v, 4) for k, v in parts["new"].items()}),
                              info=parts["info"],
                              before=dict(spread(ms_old), samples=n_old,
                                          us_per_sample=round(statistics.median(ms_old) / n_old * 1e3, 3),
                                          **{k: round(v, 4) for k, v in parts.get("old", {}).items()}))), flush=True)

    run("S1", pairs_of(256, 200, 400, "dna", 1), 16)
    rng = random.Random(5)
    s2 = ("".join(rng.choice("ACGT") for _ in range(300)), "".join(rng.choice("ACGT") for _ in range(257)))
    run("S2", [s2], 4096)
    run("S3", [(splitmix_seq(10000, 1, "dna"), splitmix_seq(10000, 2, "dna"))], 256, old_samples=32)


def count_workloads():
    def run(name, pairs):
        al = GlobalAligner(max_seq_len_prod=None, **DNA)
        a, b = [p[0] for p in pairs], [p[1] for p in pairs]
        eng, parts, last = _native.default_engine(0), [], {}

        def call():
            last["res"] = al.count_alignments(a, b)
            parts.append(eng.batch_count_timings())

        for _ in range(WARMUP):
            call()
        ms = []
        for _ in range(REPEATS):
            t0 = time.perf_counter()
            call()
            ms.append((time.perf_counter() - t0) * 1e3)
        parts, res = parts[-REPEATS:], last["res"]
        cells = sum(len(x) * len(y) for x, y in pairs)
        med = {k: round(statistics.median(x[k] for x in parts), 4) for k in parts[0]}
        count_ms, fill_ms = med["count_ms"] + med["single_count_ms"], med["words_ms"] + med["single_fill_ms"]
        print(json.dumps(dict(workload=name, pairs=len(pairs), cells=cells, ms=round(statistics.median(ms), 4),
                              ms_min=round(min(ms), 4), ms_max=round(max(ms), 4), **med,
                              count_over_fill=round(count_ms / fill_ms, 3), count_ns_per_cell=round(count_ms * 1e6 / cells, 4),
                              fill_ns_per_cell=round(fill_ms * 1e6 / cells, 4), info=eng.batch_count_info(),
                              counts_min=float(res.counts.min()), counts_max=float(res.counts.max()),
                              exact=int(res.exact.sum()))), flush=True)

    run("B1-count", pairs_of(4096, 200, 400, "dna", 1))
    run("S3-count", [(splitmix_seq(10000, 1, "dna"), splitmix_seq(10000, 2, "dna"))])


def rank_workloads():
    def run(name, pairs, nranks, options=None):
        for k, v in (options or {}).items():
            _native.OPTIONS[k] = str(v)
        al = GlobalAligner(max_seq_len_prod=None, **DNA)
        a, b = [p[0] for p in pairs], [p[1] for p in pairs]
        eng, parts, cparts, last = _native.default_engine(0), [], [], {}
        counts = al.alignments_by_rank(a, b, [()] * len(pairs)).counts
        rng = random.Random(1)
        ranks = [[rng.randrange(int(c)) for _ in range(nranks)] for c in counts]

        def call():
            last["res"] = al.alignments_by_rank(a, b, ranks)
            parts.append(eng.batch_rank_timings())

        def count():
            al.count_alignments(a, b)
            cparts.append(eng.batch_count_timings())

        for _ in range(WARMUP):
            call()
            count()
        ms = []
        for _ in range(REPEATS):
            t0 = time.perf_counter()
            call()
            ms.append((time.perf_counter() - t0) * 1e3)
            count()
        parts, cparts, res = parts[-REPEATS:], cparts[-REPEATS:], last["res"]
        cells = sum(len(x) * len(y) for x, y in pairs)
        steps = sum(nranks * (len(x) + len(y)) for x, y in pairs)
        med = {k: round(statistics.median(x[k] for x in parts), 4) for k in parts[0]}
        cmed = {"count_" + k: round(statistics.median(x[k] for x in cparts), 4) for k in cparts[0]}
        table_ms = med["table_ms"] + med["single_table_ms"]
        count_ms = cmed["count_count_ms"] + cmed["count_single_count_ms"]
        print(json.dumps(dict(workload=name, pairs=len(pairs), ranks=nranks * len(pairs), cells=cells,
                              ms=round(statistics.median(ms), 4), ms_min=round(min(ms), 4), ms_max=round(max(ms), 4), **med,
                              **cmed, table_over_count=round(table_ms / count_ms, 3),
                              table_ns_per_cell=round(table_ms * 1e6 / cells, 4),
                              walk_ms_per_mstep=round(med["walks_ms"] / steps * 1e6, 4), info=eng.batch_rank_info(),
                              saturated=int(res.saturated.sum()), options=options or {})), flush=True)
        for k in options or {}:
            del _native.OPTIONS[k]

    b1 = pairs_of(4096, 200, 400, "dna", 1)
    run("B1-rank", b1, 16)
    run("B1-rank-one-chunk", b1, 16, options={"GA_BATCH_RANK_TABLE_BYTES": 16 << 30})
    run("S3-rank", [(splitmix_seq(10000, 1, "dna"), splitmix_seq(10000, 2, "dna"))], 64)


def support_workloads():
    """B1 cut to the pairs whose dense output fits the default cap of one chunk (2 GiB) and S3's 10k x 10k pair through
    match_support, with count_alignments on the same batch in the same run: median of REPEATS after WARMUP."""
    def run(name, pairs):
        al = GlobalAligner(max_seq_len_prod=None, **DNA)
        a, b = [p[0] for p in pairs], [p[1] for p in pairs]
        eng, parts, cparts, last = _native.default_engine(0), [], [], {}

        def call():
            last["res"] = al.match_support(a, b)
            parts.append(eng.batch_support_timings())

        def count():
            al.count_alignments(a, b)
            cparts.append(eng.batch_count_timings())

        for _ in range(WARMUP):
            call()
            count()
        ms = []
        for _ in range(REPEATS):
            t0 = time.perf_counter()
            call()
            ms.append((time.perf_counter() - t0) * 1e3)
            count()
        parts, cparts, res = parts[-REPEATS:], cparts[-REPEATS:], last["res"]
        cells = sum(len(x) * len(y) for x, y in pairs)
        med = {k: round(statistics.median(x[k] for x in parts), 4) for k in parts[0]}
        cmed = {"count_" + k: round(statistics.median(x[k] for x in cparts), 4) for k in cparts[0]}
        table_ms, flow_ms = med["table_ms"] + med["single_table_ms"], med["flow_ms"] + med["single_flow_ms"]
        gather_ms = med["gather_ms"] + med["single_gather_ms"]
        count_ms = cmed["count_count_ms"] + cmed["count_single_count_ms"]
        print(json.dumps(dict(workload=name, pairs=len(pairs), cells=cells, ms=round(statistics.median(ms), 4),
                              ms_min=round(min(ms), 4), ms_max=round(max(ms), 4), **med, **cmed,
                              table_over_count=round(table_ms / count_ms, 3), flow_over_count=round(flow_ms / count_ms, 3),
                              table_ns_per_cell=round(table_ms * 1e6 / cells, 4),
                              flow_ns_per_cell=round(flow_ms * 1e6 / cells, 4),
                              gather_ns_per_cell=round(gather_ms * 1e6 / cells, 4), info=eng.batch_support_info(),
                              exact=int(res.exact.sum()),
                              core_columns=int(sum(len(res.core(k)) for k in range(min(len(pairs), 64)))))), flush=True)

    b1, out_bytes = [], 0
    for x, y in pairs_of(4096, 200, 400, "dna", 1):
        if out_bytes + len(x) * len(y) * 8 > (2 << 30):
            break
        b1.append((x, y))
        out_bytes += len(x) * len(y) * 8
    run("B1-support", b1)
    run("S3-support", [(splitmix_seq(10000, 1, "dna"), splitmix_seq(10000, 2, "dna"))])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--loop", type=int, default=0, metavar="K")
    ap.add_argument("--crossover", action="store_true")
    ap.add_argument("--align", action="store_true")
    ap.add_argument("--align-host", action="store_true")
    ap.add_argument("--align-loop", type=int, default=0, metavar="K")
    ap.add_argument("--align-crossover", action="store_true")
    ap.add_argument("--sample", action="store_true")
    ap.add_argument("--count", action="store_true")
    ap.add_argument("--rank", action="store_true")
    ap.add_argument("--support", action="store_true")
    args = ap.parse_args()
    if args.support:
        support_workloads()
    elif args.rank:
        rank_workloads()
    elif args.count:
        count_workloads()
    elif args.sample:
        sample_workloads()
    elif args.loop:
        loop(args.loop)
    elif args.align or args.align_host:
        align_workloads(device=args.align)
    elif args.align_loop:
        align_loop(args.align_loop)
    elif args.align_crossover:
        align_crossover()
    elif args.crossover:
        crossover()
    else:
        workloads()


if __name__ == "__main__":
    main()
