"""The indel-model session on the GPU (kp_ispec.h: the table, scan, track and sites kernels) against
the host session of the same per-base and per-code functions (itself pinned to an independent
oracle in tests/test_indel_model.py).  Bar: every histogram, counter, expected sum, track plane,
pattern id and resolved row equal, bit for bit; the scan path a case ran is asserted from the
session's stats."""
import numpy as np
import pytest

from kmerpapa_amd import engine, indel
from kmerpapa_amd.pattern_utils import matches
from tests import seq_ref as S

pytestmark = pytest.mark.gpu

LDS, GLOBAL = engine.ISPEC_PATH_LDS, engine.ISPEC_PATH_GLOBAL
KNOBS = ("KP_ISPEC_GLOBAL", "KP_ISPEC_LDS_P", "KP_ISPEC_GRID")
THREADS = 256
LDS_P = 8192     # KP_P_LDS_P / 2
LUT_TILE = 1024  # KP_P_LUT_TILE
RUN_LENGTHS = (63, 64, 65, 255, 256, 257, 1000)  # around one and four wave steps of the search, and many
word = engine.pattern_word

_hip_error = []


class _guard:
    """Nothing more is started on the GPU after a HIP error."""

    def __enter__(self):
        assert not _hip_error, f"an earlier GPU step failed, nothing more is started: {_hip_error[0]}"

    def __exit__(self, kind, exc, tb):
        if isinstance(exc, engine.KPError) and exc.code == -3:
            _hip_error.append(str(exc))
        return False


@pytest.fixture(scope="module")
def dev():
    with _guard():
        engine.load()
        assert engine.device_count() >= 1, "no GPU visible to the HIP runtime"
        return engine.get_device(engine.visible_devices()[0])


@pytest.fixture(scope="module")
def tile(dev):
    with _guard():
        dev.ispec_begin(2, [word("NN")], [0])
        dev.ispec_end()
        t = dev.ispec_stats()["tile"]
    assert t >= THREADS and t % THREADS == 0
    return t


def _set(monkeypatch, env):
    for key in KNOBS:
        monkeypatch.delenv(key, raising=False)
    for key, v in env.items():
        monkeypatch.setenv(key, str(v))


def _partition(rng, k, leaves, drop=0):
    """A random partition of all k-mers into at least ``leaves`` IUPAC patterns (an N becomes its
    four bases, or R and Y), ``drop`` of them left out."""
    pats = ["N" * k]
    while len(pats) < min(leaves, 4 ** k):
        i = int(rng.randint(len(pats)))
        free = [j for j, c in enumerate(pats[i]) if c in "NRY"]
        if not free:
            continue  # (a single k-mer; there is another pattern to split while there are fewer than 4^k)
        p = pats.pop(i)
        j = free[int(rng.randint(len(free)))]
        parts = {"N": ("ACGT", "RY")[int(rng.randint(2))], "R": "AG", "Y": "CT"}[p[j]]
        pats += [p[:j] + c + p[j + 1:] for c in parts]
    order = rng.permutation(len(pats))
    return [pats[i] for i in order[drop:]]


_model_cache = {}


def _model(k, n_ins, n_del, seed=0, drop=1):
    """(words, kinds, rates, names) of a random model, the kinds shuffled together; a kind with 0
    leaves has no pattern."""
    key = (k, n_ins, n_del, seed, drop)
    if key not in _model_cache:
        rng = np.random.RandomState(1000 * seed + 7 * k + n_ins)
        ins = _partition(rng, k, n_ins, drop) if n_ins else []
        dele = _partition(rng, k, n_del, drop) if n_del else []
        order = rng.permutation(len(ins) + len(dele))
        names = [(ins + dele)[i] for i in order]
        kinds = np.array([0] * len(ins) + [1] * len(dele), np.uint32)[order]
        _model_cache[key] = ([word(x) for x in names], kinds, rng.rand(len(names)) * 1e-3, names)
    return _model_cache[key]


def _session(s, k, model, seq, regions=None, track=None, sites=None, want_hist=True, rates=True, place="left", seed=0):
    """One session of one contig: (hist, other, expected, track pid, site pid, resolved, stats)."""
    words, kinds, r, _ = model
    with _guard():
        s.ispec_begin(k, words, kinds)
        try:
            h = o = e = t = p = res = None
            if regions is not None:
                h, o, e = s.ispec_regions(seq, regions, r if rates else None, want_hist)
            if track is not None:
                t = s.ispec_track(seq, *track)
            if sites is not None:
                p, res = s.ispec_sites(seq, 5, sites, place, seed)
            st = s.ispec_stats()
        finally:
            s.ispec_end()
    return h, o, e, t, p, res, st


_host_cache = {}


def _host(key, *args, **kw):
    """The host session of a case, computed once and shared by the knob settings."""
    if key not in _host_cache:
        _host_cache[key] = _session(engine.HostISpec(), *args, **kw)
    return _host_cache[key]


def _same(got, ref):
    for g, r in zip(got[:6], ref[:6]):
        assert (g is None) == (r is None)
        if g is not None:
            assert g.dtype == r.dtype and g.shape == r.shape and g.tobytes() == r.tobytes()
    for x in ("assigned", "unmatched", "invalid", "items", "tile", "lut_bytes", "sites", "sites_skipped"):
        assert got[6][x] == ref[6][x], x


def _contig(n, tile, k, seed):
    """``n`` mixed-case bases with an invalid byte k - 1 bases before and after every work-item
    boundary and around a few thread-run boundaries."""
    rng = np.random.RandomState(seed)
    seq = S.random_seq(rng, n, lower=0.25)
    run = tile // THREADS
    first = k // 2
    marks = []
    for i in (1, 2):
        b = first + i * tile
        marks += [b - (k - 1), b + (k - 1), b - k // 2 - (k - 1), b - k // 2 + 2 * (k - 1)]
    for d in range(1, k):
        b = first + (7 + 9 * d) * run
        marks += [b - d, b + 3 * run + d - 1]
    for m in marks:
        if 0 <= m < n:
            seq[m] = ord("N")
    return seq


def _regions(n, tile):
    """The whole contig, regions that start and end inside a thread's run, empty and end regions."""
    regs = [(0, n), (min(n, 5), min(n, tile // 2 + 13)), (0, 0), (max(n - 1, 0), n), (0, min(n, 1)),
            (min(n, 17), max(min(n, 17), n - 3)), (min(n, tile - 5), min(n, tile + 40)), (n, n)]
    return np.array(regs, np.uint64)


@pytest.mark.parametrize("env,path", [({}, LDS), ({"KP_ISPEC_GLOBAL": 1}, GLOBAL), ({"KP_ISPEC_GRID": 1}, LDS)],
                         ids=["lds", "global", "one_workgroup"])
def test_contig_lengths_around_the_tile(dev, tile, monkeypatch, env, path):
    """k = 4 on contigs with tile - 1, tile, tile + 1 and 2 tile + 1 windows, and one shorter than k."""
    _set(monkeypatch, env)
    k, model = 4, _model(4, 9, 7)
    for n in (tile + k - 2, tile + k - 1, tile + k, 2 * tile + k, k - 1):
        seq = _contig(n, tile, k, seed=n % 97)
        regions = _regions(n, tile)
        got = _session(dev, k, model, seq, regions)
        _same(got, _host(("len", n), k, model, seq, regions))
        if n >= k:
            assert got[6]["path"] == path and got[6]["scan_ms"] > 0 and got[6]["lut_ms"] > 0
            assert int(got[1][0, 4]) > 0 and int(got[0][0].sum()) > 3 * n and int(got[1][0, :4].min()) > 0
        else:
            assert got[6]["path"] == 0 and got[6]["items"] == 0 and got[1][:, :4].sum() == 0
        assert got[6]["lut_bytes"] == 16 * 4 ** k


def _big_model(extra):
    """k = 8: every 6-mer followed by NN an ins pattern, every 6-mer after NN a del pattern (8,192
    patterns); with ``extra`` one del pattern is split in two."""
    six = sorted(matches("NNNNNN"))
    ins = [x + "NN" for x in six]
    dele = ["NN" + x for x in six]
    if extra:
        dele = ["RN" + six[0], "YN" + six[0]] + dele[1:]
    names = ins + dele
    kinds = np.array([0] * len(ins) + [1] * len(dele), np.uint32)
    order = np.random.RandomState(5).permutation(len(names))
    names = [names[i] for i in order]
    return [word(x) for x in names], kinds[order], np.random.RandomState(6).rand(len(names)), names


def test_path_threshold(dev, tile, monkeypatch):
    """8,192 patterns run on LDS counters, 8,193 on global atomics; KP_ISPEC_LDS_P moves the bar."""
    k = 8
    seq = _contig(tile + 300, tile, k, seed=3)
    regions = np.array([(0, tile + 300), (100, 4000), (3000, tile + 5)], np.uint64)
    for extra, cases in ((0, (({}, LDS), ({"KP_ISPEC_LDS_P": 0}, GLOBAL), ({"KP_ISPEC_LDS_P": LDS_P - 1}, GLOBAL),
                              ({"KP_ISPEC_GRID": 1, "KP_ISPEC_GLOBAL": 1}, GLOBAL))),
                         (1, (({}, GLOBAL),))):
        model = _big_model(extra)
        assert len(model[0]) == LDS_P + extra
        ref = _host(("bar", extra), k, model, seq, regions)
        for env, path in cases:
            _set(monkeypatch, env)
            got = _session(dev, k, model, seq, regions)
            _same(got, ref)
            assert got[6]["path"] == path, (extra, env)
    _set(monkeypatch, {"KP_ISPEC_LDS_P": LDS_P + 1})  # the counters would not fit beside a second workgroup's
    with pytest.raises(engine.KPError) as e:
        _session(dev, k, _big_model(0), seq, regions)
    assert e.value.code == -1


def test_table_build_past_one_tile_of_patterns(dev, tile, monkeypatch):
    """Every 6-mer its own pattern for both kinds: 8,192 patterns go through the table kernel's
    staging eight tiles long, and both kinds' counters fill the LDS path to its limit."""
    _set(monkeypatch, {})
    six = sorted(matches("NNNNNN"))
    order = np.random.RandomState(8).permutation(2 * len(six))
    names = [(six + six)[i] for i in order]
    kinds = np.array([0] * len(six) + [1] * len(six), np.uint32)[order]
    model = ([word(x) for x in names], kinds, np.random.RandomState(9).rand(len(names)), names)
    assert len(names) == LDS_P > LUT_TILE
    n = tile + 777
    seq = _contig(n, tile, 6, seed=12)
    regions = np.array([(0, n), (10, 5000)], np.uint64)
    got = _session(dev, 6, model, seq, regions, track=(0, n))
    ref = _host("every6", 6, model, seq, regions, track=(0, n))
    _same(got, ref)
    assert got[6]["path"] == LDS and not got[1][:, :4].any()
    valid = ref[3][0] >= 0
    assert valid.sum() > n - 200 and (ref[3][:, valid] >= 0).all()
    # plane 1 is plane 0 of the reverse complement: both name the pattern that holds the k-mer
    assert [names[i] for i in ref[3][0][valid][:50]] == [S.revcomp(names[i]) for i in ref[3][1][valid][:50]]


@pytest.mark.parametrize("env,path", [({}, LDS), ({"KP_ISPEC_GRID": 1}, LDS), ({"KP_ISPEC_GLOBAL": 1}, GLOBAL)],
                         ids=["lds", "one_workgroup", "global"])
def test_many_short_overlapping_regions(dev, tile, monkeypatch, env, path):
    """About 2,000 regions of 1 to 40 bases in random order, with both kinds and with a kind left empty."""
    _set(monkeypatch, env)
    rng = np.random.RandomState(41)
    n = 6000
    seq = S.random_seq(rng, n, lower=0.2, invalid=0.003)
    begin = rng.randint(0, n - 40, size=2000)
    regions = np.stack([begin, begin + rng.randint(1, 41, size=2000)], axis=1).astype(np.uint64)
    for tag, model in (("both", _model(6, 40, 30)), ("ins_only", _model(6, 25, 0)), ("del_only", _model(6, 0, 25))):
        got = _session(dev, 6, model, seq, regions)
        _same(got, _host(("short", tag), 6, model, seq, regions))
        assert got[6]["path"] == path and got[6]["items"] >= 1990
        kinds = model[1]
        if tag == "ins_only":
            assert not kinds.any() and got[2][:, 2:].sum() == 0 and got[2][:, :2].sum() > 0
            assert np.array_equal(got[1][:, 2], got[1][:, 3]) and got[1][:, 2].sum() > 0
        if tag == "del_only":
            assert kinds.all() and got[2][:, :2].sum() == 0 and got[2][:, 2:].sum() > 0


def test_batching_changes_nothing(dev, tile, monkeypatch):
    _set(monkeypatch, {})
    rng = np.random.RandomState(43)
    n = 3000
    seq = S.random_seq(rng, n, lower=0.2)
    begin = rng.randint(0, n - 40, size=300)
    regions = np.stack([begin, begin + rng.randint(0, 41, size=300)], axis=1).astype(np.uint64)
    words, kinds, rates, _ = _model(4, 12, 9)
    ref = _host("batch", 4, (words, kinds, rates, None), seq, regions)
    with _guard():
        dev.ispec_begin(4, words, kinds)
        try:
            got = dev.ispec_regions(seq, regions, rates, budget=2 * len(words) * 17)
        finally:
            dev.ispec_end()
    for g, r in zip(got, ref[:3]):
        assert g.tobytes() == r.tobytes()


def test_track_planes(dev, tile, monkeypatch):
    """Four planes over a range that starts and ends mid-vector, crosses an N block and spans items."""
    _set(monkeypatch, {})
    k = 6
    n = 2 * tile + 1000
    seq = _contig(n, tile, k, seed=21)
    seq[tile - 20:tile + 31] = ord("N")
    model = _model(k, 30, 20)
    for begin, end in ((3, n - 2), (tile - 101, tile + 100), (0, n), (5, 6), (n - 3, n), (7, 7)):
        assert begin == end or (end - begin) % 4 or (begin, end) == (0, n)
        got = _session(dev, k, model, seq, track=(begin, end))
        ref = _host(("track", begin, end), k, model, seq, track=(begin, end))
        _same(got, ref)
        assert got[3].shape == (4, end - begin)
    ref = _host(("track", 3, n - 2), k, model, seq, track=(3, n - 2))[3]
    assert (ref == -2).all(axis=0).sum() >= 50 and (ref >= 0).any(axis=1).all() and (ref == -1).any()
    assert ((ref == -2).any(axis=0) == (ref == -2).all(axis=0)).all()
    _set(monkeypatch, {"KP_ISPEC_GRID": 1})
    _same(_session(dev, k, model, seq, track=(3, n - 2)), _host(("track", 3, n - 2), k, model, seq, track=(3, n - 2)))


def _run_contig():
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
    return "".join(parts), runs


def _run_sites(seq, runs):
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
            b = int(rng.randint(0, n + 1))
            copied = seq[b:b + L]
            ins = copied if len(copied) == L and set(copied.upper()) <= set("ACGT") and rng.rand() < 0.5 else \
                "".join(rng.choice(list("ACGTacgt"), size=L))
            sites.append(("ins", b, ins))
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
def run_case():
    seq, runs = _run_contig()
    sites = _run_sites(seq, runs)
    assert 19_000 < len(seq) < 21_000 and 2_900 < len(sites) < 3_600 and len(sites) % 64 and len(sites) > 1024
    arrays = engine.indel_sites([s[1] for s in sites], [s[2] if s[0] == "del" else 0 for s in sites],
                                [s[2] if s[0] == "ins" else "" for s in sites], [s[3] for s in sites])
    return np.frombuffer(seq.encode("latin-1"), np.uint8), sites, arrays


@pytest.mark.parametrize("place,seed", [("left", 0), ("right", 0), ("sample", 12), ("sample", (1 << 63) + 5)],
                         ids=["left", "right", "sample12", "sample_big_seed"])
@pytest.mark.parametrize("k", [2, 6, 10])
def test_sites_equal_the_host(dev, tile, run_case, monkeypatch, k, place, seed):
    _set(monkeypatch, {})
    seq, sites, arrays = run_case
    model = _model(k, 20, 16)
    ref = _host(("sites", k, place, seed), k, model, seq, sites=arrays, place=place, seed=seed)
    pid, res = ref[4], ref[5]
    kept = pid[:, 0] != -2
    assert 10 * int(kept.sum()) >= 9 * len(sites) and 4 * int((res[:, 1] > res[:, 0]).sum()) >= len(sites)
    assert ((pid[:, 0] == -2) == (pid[:, 1] == -2)).all() and (pid[kept] >= 0).any() and (pid[kept] == -1).any()
    span = (res[:, 1] - res[:, 0]).astype(np.int64)
    for length in RUN_LENGTHS:
        assert (span >= length - 2).sum() >= 6, length
    got = _session(dev, k, model, seq, sites=arrays, place=place, seed=seed)
    _same(got, ref)
    assert got[6]["sites"] == int(kept.sum()) and got[6]["sites_ms"] > 0
    # the counting session resolves the same sites the same way
    cres = dev.seq_count_indels(k, True, [(seq, False, 5, arrays)], place, seed)[3][0]
    assert np.array_equal(cres, got[5])


def test_sessions_exclude_each_other(dev, tile, monkeypatch):
    """kp_ispec_begin during a kp_seq, kp_pred or kp_spec session, and every holder of the arena
    during a kp_ispec session, are KP_E_STATE."""
    _set(monkeypatch, {})
    a, n3, n4 = word("NAN"), word("NNN"), word("NNNN")
    begins = {"seq": lambda: dev.seq_begin(3, True), "typed": lambda: dev.seq_begin_typed(3, True),
              "indel": lambda: dev.seq_begin_indel(4, True), "strands": lambda: dev.seq_begin_strands(4, True),
              "pred": lambda: dev.pred_begin(3, [n3], n3, False), "spec": lambda: dev.spec_begin(3, [a], [0], True),
              "ispec": lambda: dev.ispec_begin(4, [n4, n4], [0, 1])}
    ends = {"seq": lambda: dev.seq_end(False, False), "typed": lambda: dev.seq_end_typed(False, False),
            "indel": lambda: dev.seq_end_typed(False, False), "strands": lambda: dev.seq_end(False, False),
            "pred": dev.pred_end, "spec": dev.spec_end, "ispec": dev.ispec_end}
    with _guard():
        for held in begins:
            begins[held]()
            try:
                for other in ("ispec",) if held != "ispec" else tuple(begins):
                    with pytest.raises(engine.KPError) as e:
                        begins[other]()
                    assert e.value.code == -4, (held, other)
                if held == "ispec":
                    for call in (lambda: dev.greedy("NN", np.ones(16, np.uint64), np.ones(16, np.uint64), [(-1, -1, 1.0, 1.0, 1.0)]),
                                 lambda: dev.apply(2, [word("NN")], word("NN"), [0], [1], [1])):
                        with pytest.raises(engine.KPError) as e:
                            call()
                        assert e.value.code == -4
            finally:
                ends[held]()
        one = engine.indel_sites([2], [1], [""])
        for call in (lambda: dev.ispec_regions(np.zeros(5, np.uint8), [(0, 1)]), dev.ispec_end,
                     lambda: dev.ispec_track(np.zeros(5, np.uint8)), lambda: dev.ispec_sites(np.zeros(5, np.uint8), 0, one)):
            with pytest.raises(engine.KPError) as e:
                call()
            assert e.value.code == -4


def test_table_is_rebuilt_after_the_arena_grew(monkeypatch):
    """On a context of its own the arena starts at the table plus its staged patterns (4 KiB for
    k = 4).  The first sites call fits beside it, the counters of 2,000 regions do not: the arena
    grows, which frees the table, and it is built again before the scan, the track and the second
    sites call read it."""
    _set(monkeypatch, {})
    rng = np.random.RandomState(89)
    n = 333
    seq = S.random_seq(rng, n, lower=0.2)
    seq[150] = ord("N")
    begin = rng.randint(0, n - 5, size=2000)
    regions = np.stack([begin, begin + rng.randint(1, 6, size=2000)], axis=1)
    words, kinds, rates, _ = _model(4, 9, 7)
    few = engine.indel_sites([0, 151, 200, n], [1, 0, 2, 0], ["", "a", "", "CT"])

    def calls(s):
        s.ispec_begin(4, words, kinds)
        try:
            first = s.ispec_sites(seq, 1, few, "right")
            hist, other, exp = s.ispec_regions(seq, regions, rates, True)
            track = s.ispec_track(seq, 0, n)
            return first + (hist, other, exp, track) + s.ispec_sites(seq, 1, few, "right")
        finally:
            s.ispec_end()

    ref = calls(engine.HostISpec())
    with _guard():
        own = engine.Device(engine.visible_devices()[0])
        try:
            got = calls(own)
        finally:
            own.close()
    for g, r in zip(got, ref):
        assert g.dtype == r.dtype and g.shape == r.shape and g.tobytes() == r.tobytes()
    assert ref[2].nbytes > 1 << 16 and int(ref[2].sum()) > 0
    assert (ref[5] == -2).sum() >= 15 and (ref[5] >= 0).any() and (ref[0][:, 0] >= -1).any()


def test_fit_end_to_end(dev, monkeypatch, tmp_path, capsys):
    """kmerpapa-indel fit at 4-mers on a 9 kb genome, then regions --observed: the model file and the
    table equal those of the --host run byte for byte, and every kept site is found again."""
    from tests import indel_ref as R
    _set(monkeypatch, {})
    rng = np.random.RandomState(107)
    contigs = [("chr1", S.random_seq(rng, 6_000, lower=0.2, letters="AACGTT")), ("chr2", S.random_seq(rng, 3_001))]
    fa = str(tmp_path / "g.fa")
    S.write_fasta(fa, contigs)
    rows, starts, ends, n_del = [], set(), set(), 0
    for name, seq in contigs:
        text = S.text(seq)
        for s in rng.choice(np.arange(10, len(text) - 10), size=700, replace=False).tolist():
            anchor = text[s - 1].upper()
            if rng.rand() < 0.5:
                L = 1 + int(text[s].upper() in "AT")  # (more deletions at A and T: a rate that depends on the context)
                lo, _ = R.interval(text, ("del", s, L, 0))
                if (name, lo) in starts or (name, lo + L) in ends:
                    continue  # (one start and one end per breakpoint, so that no k-mer has more positives than background)
                starts.add((name, lo))
                ends.add((name, lo + L))
                rows.append(f"{name} {s} {text[s - 1:s + L].upper()} {anchor}\n")  # anchored, as a VCF spells it
                n_del += 1
            else:
                ins = "ACGT"[int(rng.randint(4))] * (1 + int(anchor in "CG"))
                lo, _ = R.interval(text, ("ins", s, ins, 0))
                if (name, lo) in starts:
                    continue
                starts.add((name, lo))
                rows.append(f"{name} {s} {anchor} {anchor}{ins}\n")
    (tmp_path / "i.txt").write_text("".join(rows))
    (tmp_path / "r.bed").write_text("chr1 0 6000\nchr2 0 3001\nchr1 1000 3000\n")
    sites, bed = str(tmp_path / "i.txt"), str(tmp_path / "r.bed")
    opts = ["-c", "3", "-a", "1", "--verbosity", "0"]
    out = {}
    with _guard():
        for host in (False, True):
            model_file, table = str(tmp_path / f"model{int(host)}.txt"), str(tmp_path / f"out{int(host)}.txt")
            extra = ["--host"] * host
            assert indel.main(["fit", fa, sites, "--radius", "2", "-o", model_file] + opts + extra) == 0
            assert indel.main(["regions", fa, "--model", model_file, "--bed", bed, "--observed", sites, "-o", table,
                               "--verbosity", "0"] + extra) == 0
            out[host] = (open(model_file).read(), open(table).read())
    assert out[False] == out[True]
    model = indel.Model.read(str(tmp_path / "model0.txt"))
    assert model.kinds == ["ins", "del"] and model.k == 4
    for kind in (0, 1):  # each kind's patterns cover every 4-mer once
        covered = sorted(kmer for x, t in zip(model.names, model.pkind.tolist()) if t == kind for kmer in matches(x))
        assert covered == sorted(matches("NNNN"))
    lines = [x.split() for x in out[False][1].splitlines()]
    col = {x: i for i, x in enumerate(lines[0])}
    assert int(lines[1][col["obs_del_start"]]) + int(lines[2][col["obs_del_start"]]) == n_del > 400
    assert int(lines[1][col["obs_ins"]]) + int(lines[2][col["obs_ins"]]) == len(rows) - n_del > 400
    assert int(lines[1][col["obs_del_end"]]) + int(lines[2][col["obs_del_end"]]) == n_del
    assert all(float(lines[1][col[c]]) > 0 for c in ("exp_ins", "exp_ins_fwd", "exp_ins_rc", "exp_del_start", "exp_del_end"))
