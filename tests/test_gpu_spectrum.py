"""The mutation spectrum on the GPU (kp_spec_lut_kernel, kp_spec_scan_kernel, kp_spec_track_kernel,
kp_spec_sites_kernel, kp_spec_sums_kernel, kp_seq_sites_typed_kernel) against the host session of
the same per-base and per-code functions (engine.HostSpec, itself pinned to an independent oracle
in tests/test_spectrum.py).  Bar: every count and id equal and ``expected`` bit-identical, on both
counter paths and every knob setting; the path a case ran is asserted from the session's stats.

Every device call of this file goes through ``_guard``: a HIP error (a fault included) is recorded
and every later test of the file fails before it starts anything on the GPU.  The guard does not
cover a kernel that hangs: the tests run in this process, as tests/test_gpu_predict.py does, so a
hang ends with the time limit of the command that runs pytest."""
import numpy as np
import pytest

from kmerpapa_amd import count as C
from kmerpapa_amd import cli, engine, spectrum
from tests import spec_ref as R

pytestmark = pytest.mark.gpu

LDS, GLOBAL = engine.SPEC_PATH_LDS, engine.SPEC_PATH_GLOBAL
KNOBS = ("KP_SPEC_GLOBAL", "KP_SPEC_LDS_P", "KP_SPEC_GRID")
THREADS = 256  # of a scan workgroup: a thread owns tile / 256 consecutive centres
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
        dev.spec_begin(1, [word("A")], [0], False)
        dev.spec_end()
        t = dev.spec_stats()["tile"]
    assert t >= THREADS and t % THREADS == 0
    return t


def _set(monkeypatch, env):
    for key in KNOBS:
        monkeypatch.delenv(key, raising=False)
    for key, v in env.items():
        monkeypatch.setenv(key, str(v))


_model_cache = {}


def _model(k, fold, n_types, leaves, seed=0, empty=None):
    """(words, ptype, rates, names) of a random model."""
    key = (k, fold, n_types, leaves, seed, empty)
    if key not in _model_cache:
        names, ptype, rates = R.random_model(np.random.RandomState(1000 * seed + 7 * k + leaves), k, fold, n_types, leaves, empty)
        _model_cache[key] = ([word(x) for x in names], ptype, rates, names)
    return _model_cache[key]


def _session(s, k, fold, model, seq, regions=None, track=None, sites=None, want_hist=True, rates=True):
    """One session of one contig: (hist, other, expected, track pid, site pid, stats)."""
    words, ptype, r, _ = model
    with _guard():
        s.spec_begin(k, words, ptype, fold)
        try:
            h = o = e = t = p = None
            if regions is not None:
                h, o, e = s.spec_regions(seq, regions, r if rates else None, want_hist)
            if track is not None:
                t = s.spec_track(seq, *track)
            if sites is not None:
                p = s.spec_sites(seq, *sites)
            st = s.spec_stats()
        finally:
            s.spec_end()
    return h, o, e, t, p, st


_host_cache = {}


def _host(key, *args, **kw):
    """The host session of a case, computed once and shared by the knob settings."""
    if key not in _host_cache:
        _host_cache[key] = _session(engine.HostSpec(), *args, **kw)
    return _host_cache[key]


def _same(got, ref):
    for g, r in zip(got[:5], ref[:5]):
        assert (g is None) == (r is None)
        if g is not None:
            assert g.dtype == r.dtype and g.shape == r.shape and g.tobytes() == r.tobytes()
    for x in ("assigned", "unmatched", "invalid", "items", "tile", "lut_bytes"):
        assert got[5][x] == ref[5][x], x


def _contig(n, tile, k, seed):
    """``n`` mixed-case bases with an invalid byte k - 1 bases before and after every work-item
    boundary and around a few thread-run boundaries."""
    rng = np.random.RandomState(seed)
    seq = R.random_seq(rng, n, lower=0.25)
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
            (min(n, 17), max(min(n, 17), n - 3)), (min(n, tile - 5), min(n, tile + 40))]
    return np.array(regs, np.uint64)


@pytest.mark.parametrize("env,path", [({}, LDS), ({"KP_SPEC_GLOBAL": 1}, GLOBAL), ({"KP_SPEC_GRID": 1}, LDS)],
                         ids=["lds", "global", "one_workgroup"])
def test_contig_lengths_around_the_tile(dev, tile, monkeypatch, env, path):
    """k = 5 with folding and six types on contigs of tile - 1, tile, tile + 1 and 2 tile + 17
    centres' worth of bases, and one shorter than k."""
    _set(monkeypatch, env)
    k, model = 5, _model(5, True, 6, 9)
    for n in (tile - 1, tile, tile + 1, 2 * tile + 17, k - 1):
        seq = _contig(n, tile, k, seed=n % 97)
        regions = _regions(n, tile)
        got = _session(dev, k, True, model, seq, regions)
        _same(got, _host(("len", n), k, True, model, seq, regions))
        if n >= k:
            assert got[5]["path"] == path and got[5]["scan_ms"] > 0 and got[5]["lut_ms"] > 0
            assert int(got[1][0, 3]) > 0 and int(got[0][0].sum()) > 2 * n
        else:
            assert got[5]["path"] == 0 and got[5]["items"] == 0 and got[1][:, :3].sum() == 0
        assert got[5]["lut_bytes"] == 16 * 4 ** k


def test_table_is_rebuilt_after_the_arena_grew(monkeypatch):
    """On a context of its own the arena starts at the table plus its staged patterns (under 2 KiB
    for k = 3).  The sites call fits in it, the counters of 2,000 regions do not: the arena grows,
    which frees the table, and it is built again before the scan, the null table, the track and
    the second sites call read it."""
    _set(monkeypatch, {})
    rng = np.random.RandomState(89)
    n = 333
    seq = R.random_seq(rng, n, lower=0.2)
    seq[150] = ord("N")
    begin = rng.randint(0, n - 5, size=2000)
    regions = np.stack([begin, begin + rng.randint(1, 6, size=2000)], axis=1)
    words, ptype, rates, _ = _model(3, True, 6, 4)
    draw = np.full(len(words), 0.05)  # (three types of a REF add up to 0.15 <= 1)
    pos, alts = np.array([0, 151, n - 1]), np.frombuffer(b"CaT", np.uint8)

    def calls(s):
        s.spec_begin(3, words, ptype, True)
        try:
            first = s.spec_sites(seq, pos, alts)
            hist, other, exp = s.spec_regions(seq, regions, rates, True)
            null = s.spec_null(seq, regions[:50], draw, 7, 2, 1, 64)
            track = s.spec_track(seq, 0, n)
            return first, hist, other, exp, null, track, s.spec_sites(seq, pos, alts)
        finally:
            s.spec_end()

    ref = calls(engine.HostSpec())
    with _guard():
        own = engine.Device(engine.visible_devices()[0])
        try:
            got = calls(own)
        finally:
            own.close()
    for g, r in zip(got, ref):
        assert g.dtype == r.dtype and g.shape == r.shape and g.tobytes() == r.tobytes()
    assert ref[1].nbytes > 1 << 16 and int(ref[1].sum()) > 0 and int(ref[4].sum()) > 0
    assert (ref[5] == -2).sum() >= 15 and (ref[5] >= 0).any()


def test_k1_twelve_types_without_folding(dev, tile, monkeypatch):
    _set(monkeypatch, {})
    model = _model(1, False, 12, 1)
    assert sorted(set(model[1])) == list(range(12))
    n = tile + 9
    seq = R.random_seq(np.random.RandomState(2), n, lower=0.5, invalid=0.01)
    regions = _regions(n, tile)
    pos = np.arange(0, n, 37)
    alts = np.frombuffer(b"ACGTtgca", np.uint8)[np.arange(pos.shape[0]) % 8]
    got = _session(dev, 1, False, model, seq, regions, track=(3, n - 2), sites=(pos, alts))
    _same(got, _host("k1", 1, False, model, seq, regions, track=(3, n - 2), sites=(pos, alts)))
    assert got[5]["path"] == LDS and set(got[4].tolist()) >= {-3, 0} and -1 not in got[4]
    # the same model with its patterns in another order: the sums kernel's per-type lists
    order = np.random.RandomState(8).permutation(12)
    mixed = ([model[0][i] for i in order], [model[1][i] for i in order], model[2][order], [model[3][i] for i in order])
    _same(_session(dev, 1, False, mixed, seq, regions), _host("k1_mixed", 1, False, mixed, seq, regions))


def test_every_kmer_its_own_pattern(dev, tile, monkeypatch):
    """k = 7, every k-mer its own pattern in all six types: 6 x 4^6 = 24,576 patterns, more than the
    16,384 the LDS counters hold, so the global path is taken without a knob."""
    _set(monkeypatch, {})
    k = 7
    names, ptype = [], []
    for t, kind in enumerate(R.types(True)):
        for code in range(4 ** 6):
            flank = "".join("ACGT"[(code >> (2 * (5 - i))) & 3] for i in range(6))
            names.append(flank[:3] + kind[0] + flank[3:])
            ptype.append(t)
    P = len(names)
    assert P == 24576 > 16384
    model = ([word(x) for x in names], ptype, R.wide_rates(np.random.RandomState(4), P), names)
    n = tile + 300
    seq = _contig(n, tile, k, seed=12)
    regions = np.array([(0, n), (tile - 9, tile + 50)], np.uint64)
    got = _session(dev, k, True, model, seq, regions, want_hist=True)
    _same(got, _host("own", k, True, model, seq, regions, want_hist=True))
    assert got[5]["path"] == GLOBAL and got[5]["lut_bytes"] == 16 * 4 ** 7
    assert got[1][:, :3].sum() == 0  # every valid window has a pattern in every slot


def test_path_threshold(dev, tile, monkeypatch):
    k, model = 5, _model(5, True, 6, 9)
    P = len(model[0])
    seq = _contig(tile + 100, tile, k, seed=5)
    regions = _regions(tile + 100, tile)
    ref = _host("thr", k, True, model, seq, regions)
    for env, path in (({"KP_SPEC_LDS_P": P}, LDS), ({"KP_SPEC_LDS_P": P - 1}, GLOBAL), ({"KP_SPEC_LDS_P": 0}, GLOBAL),
                      ({"KP_SPEC_GRID": 1, "KP_SPEC_GLOBAL": 1}, GLOBAL), ({"KP_SPEC_GRID": 3}, LDS)):
        _set(monkeypatch, env)
        got = _session(dev, k, True, model, seq, regions)
        _same(got, ref)
        assert got[5]["path"] == path, env
    _set(monkeypatch, {"KP_SPEC_LDS_P": 16385})  # the counters would not fit beside a second workgroup's
    with pytest.raises(engine.KPError) as e:
        _session(dev, k, True, model, seq, regions)
    assert e.value.code == -1


@pytest.mark.parametrize("env,path", [({}, LDS), ({"KP_SPEC_GRID": 1}, LDS), ({"KP_SPEC_GLOBAL": 1}, GLOBAL)],
                         ids=["lds", "lds_one_workgroup", "global"])
def test_many_short_overlapping_regions(dev, tile, monkeypatch, env, path):
    """2,000 regions of 1..300 bases in random order, with and without the histogram.  With one
    workgroup walking every item, counters left over from the item before, or flushed to the wrong
    row, show."""
    _set(monkeypatch, env)
    rng = np.random.RandomState(51)
    n = 2 * tile
    seq = R.random_seq(rng, n, lower=0.2, invalid=0.002)
    begin = rng.randint(2, n - 302, size=2000)
    regions = np.stack([begin, begin + rng.randint(1, 301, size=2000)], axis=1)
    k, model = 5, _model(5, True, 5, 9, empty=2)
    for want_hist in (True, False):
        got = _session(dev, k, True, model, seq, regions, want_hist=want_hist)
        _same(got, _host(("short", want_hist), k, True, model, seq, regions, want_hist=want_hist))
        assert got[5]["path"] == path and got[5]["items"] == 2000 and (got[0] is None) == (not want_hist)
    assert got[5]["unmatched"] > 0 and got[5]["assigned"] > 0


def test_table_build_past_one_tile_of_patterns(dev, tile, monkeypatch):
    """k = 9 at about 400 patterns per type: more than one LDS tile of 1,024 patterns in the build."""
    _set(monkeypatch, {})
    k, model = 9, _model(9, True, 6, 400)
    assert len(model[0]) > 2 * 1024
    n = 2 * tile + 17
    seq = _contig(n, tile, k, seed=9)
    # (short regions too: with this many patterns an item's flush is longer than its adds)
    begin = np.random.RandomState(3).randint(0, n - 2000, size=300)
    short = np.stack([begin, begin + np.random.RandomState(4).randint(1, 2000, size=300)], axis=1)
    regions = np.concatenate([_regions(n, tile), short.astype(np.uint64)])
    pos = np.random.RandomState(1).randint(0, n, size=500)
    alts = np.frombuffer(b"ACGT", np.uint8)[np.arange(500) % 4]
    got = _session(dev, k, True, model, seq, regions, track=(0, n), sites=(pos, alts))
    _same(got, _host("k9", k, True, model, seq, regions, track=(0, n), sites=(pos, alts)))
    assert got[5]["path"] == LDS and got[1][0, :3].sum() == 0 and (got[3] >= 2048).any()
    # a second session of another k on the same context: no stale table
    m5 = _model(5, True, 6, 9)
    _same(_session(dev, 5, True, m5, seq, regions), _host("k9_then_5", 5, True, m5, seq, regions))


def test_batching_changes_nothing(dev, tile, monkeypatch):
    _set(monkeypatch, {})
    words, ptype, rates, names = _model(5, True, 6, 9)
    model = spectrum.Model(names, ptype, rates)
    rng = np.random.RandomState(6)
    contigs = [("a", R.random_seq(rng, tile + 50, lower=0.1, invalid=0.001)), ("b", R.random_seq(rng, 900))]
    regions = {"a": [(0, tile + 50), (100, 400), (350, tile), (5, 5)], "b": [(0, 900), (300, 333)]}
    with _guard():
        full = spectrum.region_rates(contigs, model, regions, want_hist=True)
        small = spectrum.region_rates(contigs, model, regions, want_hist=True, budget=2 * len(names) + 1)
    host = spectrum.region_rates(contigs, model, regions, want_hist=True, host=True)
    for name in ("a", "b"):
        for x, y, z in zip(full[name], small[name], host[name]):
            assert x.tobytes() == y.tobytes() == z.tobytes()


def test_track_planes(dev, tile, monkeypatch):
    """Ranges that start and end off the 4-position alignment of the 16-byte stores."""
    _set(monkeypatch, {})
    n = 2 * tile + 3
    seq = R.random_seq(np.random.RandomState(61), n, lower=0.2, invalid=0.002)
    for k, fold, model in ((5, True, _model(5, True, 6, 9)), (2, False, _model(2, False, 12, 3, empty=5))):
        for b, e in ((0, n), (0, tile + 3), (13, tile + 7), (tile - 1, tile + 2), (5, 6), (n - 1, n), (7, 7), (n - 21, n),
                     (3, 2 * tile + 2)):
            got = _session(dev, k, fold, model, seq, track=(b, e))
            _same(got, _host(("track", k, b, e), k, fold, model, seq, track=(b, e)))
            assert got[3].shape == (3, e - b) and got[5]["items"] == -(-(e - b) // tile)
        _set(monkeypatch, {"KP_SPEC_GRID": 1})
        _same(_session(dev, k, fold, model, seq, track=(13, tile + 7)), _host(("track", k, 13, tile + 7), k, fold, model, seq, track=(13, tile + 7)))
        _set(monkeypatch, {})


def test_sites_and_typed_counting(dev, tile, monkeypatch):
    """Duplicate sites, both strands, ALT equal to REF: the site ids, and the typed counts against
    the host session."""
    _set(monkeypatch, {})
    rng = np.random.RandomState(29)
    n = tile + 9
    seq = R.random_seq(rng, n, lower=0.3, invalid=0.003)
    pos = np.concatenate([[0, 1, n - 1, n - 2], rng.randint(0, n, size=3000), [tile] * 70, [tile - 1] * 3])
    alts = np.frombuffer(b"ACGTacgt", np.uint8)[rng.randint(0, 8, size=pos.shape[0])]
    for k, fold, model in ((5, True, _model(5, True, 6, 9)), (3, False, _model(3, False, 12, 4)), (1, True, _model(1, True, 6, 1))):
        got = _session(dev, k, fold, model, seq, sites=(pos, alts))
        _same(got, _session(engine.HostSpec(), k, fold, model, seq, sites=(pos, alts)))
        assert {-3, -2} <= set(got[4].tolist()) and (got[4] >= 0).sum() > 1500 and got[5]["path"] == 0
        jobs = [(seq, None, (pos, alts)), (seq[:k - 1], None, None), (seq[100:900], [(5, 700)], (pos[:50] % 800, alts[:50]))]
        with _guard():
            dp, db, dst = dev.seq_count_typed(k, fold, jobs)
        hp, hb, hst = engine.HostSpec().seq_count_typed(k, fold, jobs)
        assert dp.tobytes() == hp.tobytes() and db.tobytes() == hb.tobytes() and int(dp.sum()) == hst["sites"] > 2000
        for x in ("windows", "windows_invalid", "sites", "sites_skipped", "items"):
            assert dst[x] == hst[x], x
    with _guard():
        dev.seq_begin_typed(3, True)
        try:
            for call in (lambda: dev.seq_sites(seq, [1]), lambda: dev.seq_end()):
                with pytest.raises(engine.KPError) as e:
                    call()
                assert e.value.code == -4
            with pytest.raises(engine.KPError) as e:
                dev.seq_sites_typed(seq, [1, 2], b"AN")
            assert e.value.code == -1
        finally:
            dev.seq_end_typed(False, False)


def test_sessions_exclude_each_other(dev, tile, monkeypatch):
    """kp_spec_begin during a kp_seq or kp_pred session, and every holder of the arena during a
    kp_spec session, are KP_E_STATE."""
    _set(monkeypatch, {})
    a, n3 = word("NAN"), word("NNN")
    begins = {"seq": lambda: dev.seq_begin(3, True), "typed": lambda: dev.seq_begin_typed(3, True),
              "pred": lambda: dev.pred_begin(3, [n3], n3, False), "spec": lambda: dev.spec_begin(3, [a], [0], True)}
    ends = {"seq": lambda: dev.seq_end(False, False), "typed": lambda: dev.seq_end_typed(False, False),
            "pred": dev.pred_end, "spec": dev.spec_end}
    with _guard():
        for held in ("seq", "typed", "pred", "spec"):
            begins[held]()
            try:
                for other in ("spec",) if held != "spec" else ("seq", "typed", "pred", "spec"):
                    with pytest.raises(engine.KPError) as e:
                        begins[other]()
                    assert e.value.code == -4, (held, other)
                if held == "spec":
                    for call in (lambda: dev.greedy("NN", np.ones(16, np.uint64), np.ones(16, np.uint64), [(-1, -1, 1.0, 1.0, 1.0)]),
                                 lambda: dev.apply(2, [word("NN")], word("NN"), [0], [1], [1])):
                        with pytest.raises(engine.KPError) as e:
                            call()
                        assert e.value.code == -4
            finally:
                ends[held]()
        for call in (lambda: dev.spec_regions(np.zeros(5, np.uint8), [(0, 1)]), dev.spec_end):
            with pytest.raises(engine.KPError) as e:
                call()
            assert e.value.code == -4


def test_fit_end_to_end(dev, monkeypatch, tmp_path, capsys):
    """kmerpapa-spectrum fit at 5-mers on a 20 kb genome with 2,000 sites: every type's partition
    is what the existing kmerpapa writes for the count files, and regions --observed finds every
    accepted site."""
    _set(monkeypatch, {})
    rng = np.random.RandomState(37)
    contigs = [("chr1", R.random_seq(rng, 14_011, lower=0.3, invalid=0.002, letters="AACGTTT")), ("chr2", R.random_seq(rng, 6_000))]
    fa = str(tmp_path / "g.fa")
    R.write_fasta(fa, contigs)
    rows = []
    for name, seq in contigs:
        cg = np.flatnonzero(np.isin(seq & 0xDF, (ord("C"), ord("G"))))
        for p in np.concatenate([rng.choice(cg, size=400, replace=False), rng.choice(seq.shape[0], size=600, replace=False)]):
            ref = chr(seq[p]).upper()
            if ref in "ACGT":
                rows.append((name, int(p) + 1, ref, "ACGT"[("ACGT".index(ref) + 1 + rng.randint(3)) % 4]))
    with open(tmp_path / "m.txt", "w") as f:
        f.write("".join(f"{c} {p} {r} {a}\n" for c, p, r, a in rows))
    sites, prefix, model_file = str(tmp_path / "m.txt"), str(tmp_path / "fit"), str(tmp_path / "model.txt")
    opts = ["-c", "3", "5", "-a", "0.5", "1", "-N", "2", "--seed", "1"]
    with _guard():
        assert spectrum.main(["fit", fa, sites, "-k", "5", "-o", model_file, "--prefix", prefix, "--verbosity", "0"] + opts) == 0
        model = spectrum.Model.read(model_file)
        assert model.types == R.types(True) and model.k == 5
        assert spectrum.main(["count", fa, sites, "-k", "5", "-o", str(tmp_path / "c"), "--verbosity", "0"]) == 0
        for kind in model.types:
            tag = f"{kind[0]}_{kind[2]}"
            assert open(f"{prefix}.{tag}.txt").read() == open(tmp_path / f"c.{tag}.txt").read()
            one = str(tmp_path / "one.txt")
            assert C.main(["snv", fa, sites, "--type", kind, "-k", "5", "-o", one, "--verbosity", "0"]) == 0
            assert open(one).read() == open(f"{prefix}.{tag}.txt").read()
            part = str(tmp_path / "part.txt")
            assert cli.main(["-p", f"{tmp_path}/c.{tag}.txt", "-b", f"{tmp_path}/c.background.txt", "-s", "NN" + kind[0] + "NN",
                             "-o", part, "--verbosity", "0"] + opts) == 0
            import gc
            gc.collect()  # (the output file of cli.main is closed with its argparse namespace)
            assert open(part).read() == open(f"{prefix}.{tag}.partition.txt").read() != ""
        with open(tmp_path / "r.bed", "w") as f:
            f.write("chr1 0 14011\nchr2 0 6000\nchr1 1000 3000\n")
        out = str(tmp_path / "out.txt")
        capsys.readouterr()
        assert spectrum.main(["regions", fa, "--model", model_file, "--bed", str(tmp_path / "r.bed"), "--observed", sites,
                              "-o", out]) == 0
        host_out = str(tmp_path / "host.txt")
        assert spectrum.main(["regions", fa, "--model", model_file, "--bed", str(tmp_path / "r.bed"), "--observed", sites,
                              "-o", host_out, "--verbosity", "0"], host=True) == 0
    assert open(out).read() == open(host_out).read()
    lines = [x.split() for x in open(out).read().splitlines()]
    col = lines[0].index("obs_total")
    assert int(lines[1][col]) + int(lines[2][col]) == len(rows) > 1900
    assert float(lines[1][lines[0].index("exp_total")]) > 0
