"""Indel breakpoint counts on the GPU (kp_seq_indels_kernel and the both-strand builds of
kp_seq_scan_kernel) against the host session of the same per-base code (itself pinned to an
independent oracle and to the brute-force definition in tests/test_indel.py).  Bar: the four
tables, every resolved row and every count stat equal, bit for bit; the scan path a case ran is
asserted from the session's stats."""
import gc

import numpy as np
import pytest

from kmerpapa_amd import cli, engine
from kmerpapa_amd import count as C
from kmerpapa_amd.pattern_utils import matches
from tests import indel_ref as R
from tests import seq_ref as S

pytestmark = pytest.mark.gpu

LDS, GLOBAL = engine.SEQ_PATH_LDS, engine.SEQ_PATH_GLOBAL
KNOBS = ("KP_SEQ_GLOBAL", "KP_SEQ_LDS_K", "KP_SEQ_GRID", "KP_SEQ_MERGE", "KP_SEQ_BOTH_STEPS")
RUN_LENGTHS = (63, 64, 65, 255, 256, 257, 1000)  # around one and four wave steps of the search, and many


@pytest.fixture(scope="module")
def dev():
    engine.load()
    assert engine.device_count() >= 1, "no GPU visible to the HIP runtime"
    return engine.get_device(engine.visible_devices()[0])


def _set(monkeypatch, env):
    for key in KNOBS:
        monkeypatch.delenv(key, raising=False)
    for key, v in env.items():
        monkeypatch.setenv(key, str(v))


def _contig():
    """About 20,000 bases: random mixed-case sequence around homopolymer and dinucleotide runs of
    RUN_LENGTHS, an N block, a run touching each end.  Returns ``(seq, runs)``, runs as ``(start,
    length, unit)``; every run is flanked by G, which no unit holds."""
    rng = np.random.RandomState(101)
    parts, runs, at = [], [], 0

    def put(text):
        nonlocal at
        parts.append(text)
        at += len(text)

    def run(unit, length):
        runs.append((at, length, unit))
        put((unit * length)[:length])

    def spacer(n):
        put("G" + S.text(S.random_seq(rng, n, lower=0.2)) + "G")

    run("A", 70)  # touches position 0
    spacer(300)
    for i, length in enumerate(RUN_LENGTHS):
        run("AT"[i % 2], length)
        spacer(500)
        run(("CA", "TC")[i % 2], length)
        spacer(500)
    put("N" * 50)
    spacer(2500)
    run("t", 300)  # lower case
    spacer(int(19_900 - at))
    run("CT", 91)  # touches n
    seq = "".join(parts)
    return seq, runs


def _sites(seq, runs):
    """About 3,000 sites, not a multiple of 64: in every run at its start, middle and end insertions
    of one unit, of 3, 64 and 70 bases and deletions of 1, 2 and (long runs) 300; random indels;
    duplicates; sites at the contig's ends and around the N block, which get skipped."""
    rng = np.random.RandomState(103)
    n = len(seq)
    sites = []
    for start, length, unit in runs:
        for at in (start, start + length // 2, start + length):
            phase = unit[(at - start) % len(unit):] + unit[:(at - start) % len(unit)]  # the unit as it reads at `at`
            for L in (len(unit), 3, 64, 70):
                sites.append(("ins", at, (phase * L)[:L]))
            sites.append(("ins", at, "G"))  # breaks the run: unambiguous
            for L in (1, 2) + ((300,) if length >= 1000 else ()):
                if at + L <= n:
                    sites.append(("del", at, L))
                if at - L >= 0:
                    sites.append(("del", at - L, L))
    for _ in range(2600):
        L = int(rng.choice((1, 1, 2, 3)))
        if rng.rand() < 0.5:
            sites.append(("ins", int(rng.randint(0, n + 1)), "".join(rng.choice(list("ACGTacgt"), size=L))))
        else:
            L = min(L, 2)
            sites.append(("del", int(rng.randint(0, n - L + 1)), L))
    block = seq.index("N" * 50)
    for at in (0, 1, 2, 3, n, n - 1, n - 2, n - 3, block - 1, block, block + 1, block + 25, block + 50, block + 51):
        sites += [("ins", at, "A"), ("ins", at, "CT")]
        if at < n:
            sites.append(("del", at, 1))
    sites += sites[5:40]  # duplicates
    sites.append(("del", 0, n))  # the whole contig
    keys = rng.randint(0, 1 << 62, size=len(sites)).tolist()
    keys[7] = keys[8]  # (two sites, one key)
    return [s + (key,) for s, key in zip(sites, keys)]


@pytest.fixture(scope="module")
def case():
    seq, runs = _contig()
    sites = _sites(seq, runs)
    assert 19_000 < len(seq) < 21_000 and 2_900 < len(sites) < 3_600 and len(sites) % 64 and len(sites) > 1024
    arrays = engine.indel_sites([s[1] for s in sites], [s[2] if s[0] == "del" else 0 for s in sites],
                                [s[2] if s[0] == "ins" else "" for s in sites], [s[3] for s in sites])
    # regions that start and end inside runs, one that ends where the next begins
    r = {length: start for start, length, unit in runs if unit == "A" or unit == "T"}
    regions = np.array([(5, 40), (r[255] + 100, r[256] + 7), (r[256] + 7, r[256] + 200), (r[1000] + 500, r[1000] + 501),
                        (len(seq) - 30, len(seq))])
    return np.frombuffer(seq.encode("latin-1"), np.uint8), seq, sites, arrays, regions


_host_cache = {}


def _host(case, k, both, place, seed, regions=None):
    key = (k, both, place, seed, regions is None)
    if key not in _host_cache:
        _host_cache[key] = engine.HostSeq().seq_count_indels(k, both, [(case[0], regions, 5, case[3])], place, seed)
    return _host_cache[key]


def _same(got, ref):
    assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1])
    assert {x: got[2][x] for x in S.COUNT_STATS} == {x: ref[2][x] for x in S.COUNT_STATS}
    assert got[2]["items"] == ref[2]["items"]
    assert len(got[3]) == len(ref[3]) == 1 and np.array_equal(got[3][0], ref[3][0])


def test_the_case_holds_what_it_should(case):
    """The host session of the case (pinned to the oracle on a slice of it): long intervals of every
    run length, skipped sites, and the oracle's own rows for the sites inside the first runs."""
    ref = _host(case, 4, True, "left", 0)
    res, st = ref[3][0], ref[2]
    span = (res[:, 1] - res[:, 0]).astype(np.int64)
    for length in RUN_LENGTHS:
        assert (span >= length - 2).sum() >= 6, length
    assert span.max() >= 1000 and st["sites_skipped"] > 20 and st["sites"] > 2800
    assert st["sites"] + st["sites_skipped"] == len(case[2])
    head = [i for i, s in enumerate(case[2]) if s[1] + (s[2] if s[0] == "del" else 0) < 2000][:150]
    assert len(head) == 150
    for place, seed in (("left", 0), ("right", 0), ("sample", 12)):
        rows = _host(case, 4, True, place, seed)[3][0]
        for i in head:
            lo, hi = R.interval(case[1], case[2][i])
            assert rows[i].tolist() == [lo, hi, R.place(lo, hi, place, seed, 5, case[2][i][3])], (i, case[2][i])


@pytest.mark.parametrize("place,seed", [("left", 0), ("right", 0), ("sample", 12), ("sample", (1 << 63) + 5)],
                         ids=["left", "right", "sample12", "sample_big_seed"])
@pytest.mark.parametrize("both", [True, False], ids=["both", "forward"])
@pytest.mark.parametrize("k,path", [(2, LDS), (4, LDS), (6, LDS), (8, GLOBAL)])
def test_device_equals_host(dev, case, monkeypatch, k, path, both, place, seed):
    _set(monkeypatch, {})
    got = dev.seq_count_indels(k, both, [(case[0], None, 5, case[3])], place, seed)
    _same(got, _host(case, k, both, place, seed))
    assert got[2]["path"] == path and got[2]["scan_ms"] > 0
    if both:
        assert int(got[1].sum()) == 2 * got[2]["windows"]


@pytest.mark.parametrize("both", [True, False], ids=["both", "forward"])
@pytest.mark.parametrize("k,env,path", [(4, {"KP_SEQ_GLOBAL": 1}, GLOBAL), (4, {"KP_SEQ_MERGE": 0}, LDS),
                                        (4, {"KP_SEQ_GLOBAL": 1, "KP_SEQ_MERGE": 0}, GLOBAL), (8, {"KP_SEQ_MERGE": 0}, GLOBAL),
                                        (6, {"KP_SEQ_GRID": 1, "KP_SEQ_BOTH_STEPS": 1}, LDS),
                                        (4, {"KP_SEQ_GRID": 2, "KP_SEQ_BOTH_STEPS": 1}, LDS),
                                        (6, {"KP_SEQ_GRID": 1}, LDS)],
                         ids=["global4", "lds4_merge0", "global4_unmerged", "global8_unmerged", "lds6_three_launches",
                              "lds4_two_launches", "lds6_one_workgroup"])
def test_scan_knobs(dev, case, monkeypatch, k, env, path, both):
    _set(monkeypatch, env)
    got = dev.seq_count_indels(k, both, [(case[0], None, 5, case[3])], "left", 0)
    _same(got, _host(case, k, both, "left", 0))
    assert got[2]["path"] == path and got[2]["items"] == 3


@pytest.mark.parametrize("k,path", [(4, LDS), (8, GLOBAL)])
def test_regions_inside_runs(dev, case, monkeypatch, k, path):
    _set(monkeypatch, {})
    for both in (True, False):
        got = dev.seq_count_indels(k, both, [(case[0], case[4], 5, case[3])], "right", 0)
        _same(got, _host(case, k, both, "right", 0, regions=case[4]))
        assert got[2]["path"] == path and 0 < got[2]["windows"] < 2000


def test_background_only_sessions(dev, case, monkeypatch):
    """kp_seq_begin_strands: one column, any k; both strands or the forward strand unfolded."""
    host = engine.HostSeq()
    for k, env, path in ((3, {}, LDS), (7, {}, LDS), (7, {"KP_SEQ_GLOBAL": 1}, GLOBAL), (9, {}, GLOBAL), (8, {}, GLOBAL)):
        for both in (True, False):
            _set(monkeypatch, env)
            jobs = [(case[0], None), (case[0][:5000], case[4][:1])]
            bg, st = dev.seq_count_strands(k, both, jobs)
            ref, rst = host.seq_count_strands(k, both, jobs)
            assert np.array_equal(bg, ref) and st["windows"] == rst["windows"] and st["path"] == path
            assert int(bg.sum()) == (2 if both else 1) * st["windows"]
    with_cols = _host(case, 8, True, "left", 0)[1]
    assert np.array_equal(dev.seq_count_strands(8, True, [(case[0], None)])[0], with_cols)


def test_two_contigs_and_a_second_session(dev, case, monkeypatch):
    """Two contigs in one session (each with its own index), then a session of another k on the
    same arena: the tables are zeroed again."""
    _set(monkeypatch, {})
    short = case[0][:3000]
    few = engine.indel_sites([10, 500, 2990, 3000], [1, 0, 2, 0], ["", "ag", "", "T"], [1, 2, 3, 4])
    jobs = [(case[0], None, 0, case[3]), (short, None, 1, few), (short, False, 2, few)]
    for k in (6, 8, 4):
        got = dev.seq_count_indels(k, True, jobs, "sample", 3)
        ref = engine.HostSeq().seq_count_indels(k, True, jobs, "sample", 3)
        assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1])
        assert {x: got[2][x] for x in S.COUNT_STATS} == {x: ref[2][x] for x in S.COUNT_STATS}
        assert all(np.array_equal(a, b) for a, b in zip(got[3], ref[3])) and len(got[3]) == 3


def test_error_calls_on_the_device(dev, case, monkeypatch):
    _set(monkeypatch, {})
    seq = case[0][:100]
    one = engine.indel_sites([80], [1], [""])  # (in random sequence, every window valid)
    for k in (3, 0, 16):
        with pytest.raises(engine.KPError) as e:
            dev.seq_begin_indel(k)
        assert e.value.code == -1
    with pytest.raises(engine.KPError) as e:
        dev.seq_indels(seq, 0, one)
    assert e.value.code == -4
    dev.seq_begin_indel(4)
    try:
        for call in (lambda: dev.seq_sites(seq, [1]), lambda: dev.seq_sites_typed(seq, [1], b"C"),
                     lambda: dev.seq_begin_indel(4), lambda: dev.seq_begin(3)):
            with pytest.raises(engine.KPError) as e:
                call()
            assert e.value.code == -4
        for bad in (engine.indel_sites([101], [0], ["A"]), engine.indel_sites([99], [2], [""]),
                    engine.indel_sites([5], [0], [""]), engine.indel_sites([5], [1], ["A"]),
                    engine.indel_sites([5, 6], [0, 0], ["A", "AN"])):
            with pytest.raises(engine.KPError) as e:
                dev.seq_indels(seq, 0, bad)
            assert e.value.code == -1
        with pytest.raises(KeyError):
            dev.seq_indels(seq, 0, one, place="middle")
        assert dev.seq_stats()["sites"] == 0 and dev.seq_stats()["sites_skipped"] == 0  # (nothing was launched)
        dev.seq_indels(seq, 0, one)
    finally:
        cols, bg = dev.seq_end_typed()
    assert int(cols.sum()) == 4 and not bg.any()
    dev.seq_begin_strands(5, True)
    try:
        for call in (lambda: dev.seq_sites(seq, [1]), lambda: dev.seq_indels(seq, 0, one)):
            with pytest.raises(engine.KPError) as e:
                call()
            assert e.value.code == -4
    finally:
        dev.seq_end(False, False)


def test_command_line_to_a_fitted_partition(dev, monkeypatch, tmp_path, capsys):
    """kmerpapa-count indel and background --strands both at k = 4 on the GPU write what the host
    path writes, and the main program fits the pair: the printed partition covers every 4-mer once."""
    _set(monkeypatch, {})
    rng = np.random.RandomState(107)
    contigs = [("chr1", S.random_seq(rng, 6_000, lower=0.2, letters="AACGTT")), ("chr2", S.random_seq(rng, 3_001))]
    fa = str(tmp_path / "g.fa")
    S.write_fasta(fa, contigs)
    rows, starts, ends = [], set(), set()
    for name, seq in contigs:
        text = S.text(seq)
        for s in rng.choice(np.arange(10, len(text) - 10), size=500, replace=False).tolist():
            L = 1 + int(text[s].upper() in "AT")  # (more deletions at A and T: a rate that depends on the context)
            lo, _ = R.interval(text, ("del", s, L, 0))
            if (name, lo) in starts or (name, lo + L) in ends:
                continue  # (one start and one end per breakpoint, so that no k-mer has more positives than background)
            starts.add((name, lo))
            ends.add((name, lo + L))
            rows.append(f"{name} {s} {text[s - 1:s + L].upper()} {text[s - 1].upper()}\n")  # anchored, as a VCF spells it
    (tmp_path / "d.txt").write_text("".join(rows))
    out = {}
    for host in (False, True):
        for tag, argv in (("del", ["indel", fa, str(tmp_path / "d.txt"), "del_start", "--radius", "2", "--resolved",
                                   str(tmp_path / f"res{int(host)}.txt")]),
                          ("bg", ["background", fa, "-k", "4", "--strands", "both"])):
            path = str(tmp_path / f"{tag}{int(host)}.txt")
            assert C.main(argv + ["-o", path, "--verbosity", "0"], host=host) == 0
            out[tag, host] = open(path).read()
    assert out["del", False] == out["del", True] and out["bg", False] == out["bg", True]
    assert open(tmp_path / "res0.txt").read() == open(tmp_path / "res1.txt").read()
    assert len(open(tmp_path / "res0.txt").read().splitlines()) == len(rows) > 600
    assert sum(int(x.split()[1]) for x in out["del", False].splitlines()) == 2 * len(rows)
    part = str(tmp_path / "part.txt")
    assert cli.main(["-p", str(tmp_path / "del0.txt"), "-b", str(tmp_path / "bg0.txt"), "-c", "3", "-a", "1", "-o", part,
                     "--verbosity", "0"]) == 0
    gc.collect()  # (the output file of cli.main is closed with its argparse namespace)
    lines = [x.split() for x in open(part).read().splitlines()]
    assert lines[0] == ["pattern", "p_neg", "p_pos", "p_rate"] and len(lines) > 1
    covered = sorted(kmer for row in lines[1:] for kmer in matches(row[0]))
    assert covered == sorted(matches("NNNN"))
    assert sum(int(row[2]) for row in lines[1:]) == 2 * len(rows)
