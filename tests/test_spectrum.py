"""The whole mutation spectrum in one pass (kmerpapa_amd.spectrum, kp_spec.h) on the host session
(engine.HostSpec: the kernels' per-base and per-code functions run serially) against the
independent oracle tests/spec_ref.py, pinned to the existing single-type code (engine.HostPred,
engine.seq_host, kmerpapa-count), with the error codes and the command line.  Every comparison is
exact equality."""
import io

import numpy as np
import pytest

from kmerpapa_amd import count as C
from kmerpapa_amd import engine, spectrum
from tests import spec_ref as R

word = engine.pattern_word
ARG, STATE = -1, -4


def _model(seed, k, fold, n_types, leaves, empty=None):
    names, ptype, rates = R.random_model(np.random.RandomState(seed), k, fold, n_types, leaves, empty)
    return names, ptype, rates


def _regions(n):
    """Empty, overlapping, duplicated regions, and ones that touch both contig ends."""
    regs = [(0, n), (0, 0), (n, n), (0, min(n, 3)), (max(n - 2, 0), n), (n // 3, n // 2 + 1), (n // 3, n // 2 + 1),
            (n // 4, n - n // 4)]
    return np.array([(b, min(max(b, e), n)) for b, e in regs], np.uint64)


def _alts(rng, seq, pos):
    """A forward-strand ALT per site, now and then equal to the base there, in either case."""
    alts = np.frombuffer(b"ACGTacgt", np.uint8)[rng.randint(0, 8, size=len(pos))].copy()
    same = rng.random_sample(len(pos)) < 0.1
    base = seq[np.asarray(pos, np.intp)]
    ok = np.isin(base & 0xDF, list(b"ACGT"))
    alts[same & ok] = base[same & ok]
    return alts


CASES = [(1, False, 12, 1), (1, True, 6, 1), (2, False, 12, 3), (3, True, 6, 5), (3, False, 12, 4), (5, True, 6, 9),
         (5, False, 12, 7), (5, True, 3, 9), (5, True, 1, 9), (3, False, 3, 4), (3, False, 1, 4)]


@pytest.mark.parametrize("k,fold,n_types,leaves", CASES, ids=[f"k{c[0]}_fold{int(c[1])}_T{c[2]}" for c in CASES])
def test_host_session_equals_the_oracle(k, fold, n_types, leaves):
    rng = np.random.RandomState(100 * k + n_types + fold)
    names, ptype, rates = _model(k + n_types, k, fold, n_types, leaves, empty=1 if n_types > 3 else None)
    assert len(set(ptype)) == (n_types - 1 if n_types > 3 else n_types)
    words = [word(x) for x in names]
    for n in (0, k - 1, k, 2 * k + 3, 300):
        seq = R.random_seq(rng, n, lower=0.3, invalid=0.03 if n > 20 else 0.0)
        if n == 2 * k + 3:
            seq[k] = ord("n")
        regs = _regions(n)
        pos = rng.randint(0, n, size=40) if n else np.zeros(0, np.int64)
        alts = _alts(rng, seq, pos)
        tb, te = (n // 5, n - n // 7)
        hist, other, exp, tpid, spid, st = engine.spec_host(k, words, ptype, fold, seq, regs, rates, (tb, te), (pos, alts))
        rh, ro, re = R.regions(seq, names, ptype, fold, regs.tolist(), rates)
        assert np.array_equal(hist, rh) and np.array_equal(other, ro)
        assert exp.tobytes() == re.tobytes()
        assert np.array_equal(tpid, R.track(seq, names, ptype, fold, tb, te))
        assert np.array_equal(spid, R.sites(seq, names, ptype, fold, pos, alts))
        # the row identity: per region and slot, the slot's patterns, its misses and the invalid centres
        for s in range(3):
            cols = [p for p in range(len(names)) if ptype[p] % 3 == s]
            total = hist[:, cols].sum(axis=1) + other[:, s] + other[:, 3]
            assert np.array_equal(total, regs[:, 1] - regs[:, 0])
        assert st["assigned"] == int(hist.sum()) and st["invalid"] == int(other[:, 3].sum())
        assert st["lut_bytes"] == 16 * 4 ** k and st["path"] == 0
        # the session calls one by one give what the one-call form gives
        s = engine.HostSpec()
        s.spec_begin(k, words, ptype, fold)
        try:
            h2, o2, e2 = s.spec_regions(seq, regs, rates)
            assert h2.tobytes() == hist.tobytes() and o2.tobytes() == other.tobytes() and e2.tobytes() == exp.tobytes()
            assert s.spec_regions(seq, regs, None, want_hist=False)[0] is None
            assert np.array_equal(s.spec_track(seq, tb, te), tpid) and np.array_equal(s.spec_sites(seq, pos, alts), spid)
        finally:
            s.spec_end()


@pytest.mark.parametrize("k,fold", [(3, True), (5, True), (5, False), (2, False)])
def test_every_type_equals_the_single_partition_session(k, fold):
    """Pinned to kp_pred: the columns of a type are HostPred's histogram of that partition alone,
    and its expected count is bit-identical."""
    rng = np.random.RandomState(7 + k)
    names, ptype, rates = _model(3, k, fold, 6 if fold else 12, 6, empty=2)
    seq = R.random_seq(rng, 700, lower=0.2, invalid=0.01)
    regs = _regions(700)
    hist, other, exp, tpid, _, _ = engine.spec_host(k, [word(x) for x in names], ptype, fold, seq, regs, rates, (0, 700))
    ptype = np.array(ptype)
    for t in range(12):
        cols = np.flatnonzero(ptype == t)
        if not cols.shape[0]:
            assert not exp[:, t].any()
            continue
        sub = [names[i] for i in cols]
        sw = word("N" * (k // 2) + R.ALL_TYPES[t][0] + "N" * (k - 1 - k // 2))
        h1, o1, e1, t1, _, _ = engine.pred_host(k, [word(x) for x in sub], sw, fold, seq, regs, rates[cols], (0, 700))
        assert np.array_equal(hist[:, cols], h1) and exp[:, t].tobytes() == e1.tobytes()
        assert np.array_equal(other[:, 3], o1[:, 1])
        own = tpid[t % 3]
        assert np.array_equal(np.where(np.isin(own, cols), own - cols[0], np.where(own == -2, -2, -1)), t1)


@pytest.mark.parametrize("k,fold", [(1, True), (3, True), (5, True), (5, False), (2, False)])
def test_typed_counts(k, fold):
    rng = np.random.RandomState(11 + k)
    contigs = [R.random_seq(rng, 400, lower=0.3, invalid=0.02), R.random_seq(rng, k - 1), R.random_seq(rng, 90)]
    jobs = []
    for seq in contigs:
        n = seq.shape[0]
        pos = np.concatenate([rng.randint(0, n, size=150), [0, n - 1, n // 2, n // 2]]) if n else np.zeros(0, np.int64)
        jobs.append((seq, None, (pos, _alts(rng, seq, pos))))
    pos, bg, st = engine.HostSpec().seq_count_typed(k, fold, jobs)
    rpos, rbg, rst = R.typed_counts(k, fold, jobs)
    for s in range(3):
        assert np.array_equal(pos[s], R.dense(rpos[s], k))
    assert np.array_equal(bg, R.dense(rbg, k))
    for x in ("windows", "windows_invalid", "sites", "sites_skipped"):
        assert st[x] == rst[x], x
    assert st["sites_skipped"] > 0 and st["sites"] > 100
    # pinned to kp_seq: slot s restricted to centre X = the plain session of the sites of type X>Y
    for kind in R.types(fold):
        plain = []
        for seq, _, (p, a) in jobs:
            s = R.text(seq)
            keep = []
            for x, y in zip(p.tolist(), a.tolist()):
                ref, alt = s[x].upper(), chr(y).upper()
                if ref in "ACGT" and ref != alt:
                    if fold and ref in "GT":
                        ref, alt = R.COMPLEMENT[ref], R.COMPLEMENT[alt]
                    if ref + ">" + alt == kind:
                        keep.append(x)
            plain.append((seq, False, np.array(keep, np.uint64)))
        one, _, _ = engine.seq_host(k, fold, plain)
        assert np.array_equal(spectrum.type_column(k, pos, kind), one), kind
    tables = spectrum.tables_of(k, fold, pos * 0, bg)
    assert sorted(tables) == sorted(R.types(fold)) and sum(int(t.U.sum()) for t in tables.values()) == 3 * int(bg.sum())
    with pytest.raises(ValueError, match="background counts should be larger"):
        spectrum.tables_of(k, fold, pos + np.uint64(10 ** 6), bg)


def _raises(code, call, text=None):
    with pytest.raises(engine.KPError) as e:
        call()
    assert e.value.code == code, str(e.value)
    if text is not None:
        assert text in str(e.value), str(e.value)


def test_errors():
    s = engine.HostSpec()
    seq = R.random_seq(np.random.RandomState(1), 50)
    _raises(ARG, lambda: s.spec_begin(3, [word("NMN")], [3], True), "centre of pattern 0")
    _raises(ARG, lambda: s.spec_begin(3, [word("NAN"), word("NCN")], [0, 1], True), "centre of pattern 1")
    _raises(ARG, lambda: s.spec_begin(3, [word("NCN"), word("AAN"), word("ACT"), word("MCN")], [3, 0, 3, 3], True),
            "patterns 0 and 2 share k-mers")
    _raises(ARG, lambda: s.spec_begin(3, [word("NAN"), word("ACT"), word("MCN")], [0, 4, 4], True),
            "patterns 1 and 2 share k-mers")
    _raises(ARG, lambda: s.spec_begin(3, [word("NAN")], [12], False), "type 12")
    _raises(ARG, lambda: s.spec_begin(3, [word("NGN")], [6], True), "type 6")
    _raises(ARG, lambda: s.spec_begin(2, [word("NA")], [0], True), "odd k")
    _raises(ARG, lambda: s.spec_begin(0, [word("A")], [0], False))
    _raises(ARG, lambda: s.spec_begin(16, [word("N" * 8 + "A" + "N" * 7)], [0], False))
    _raises(ARG, lambda: s.spec_begin(3, [], [], True), "no patterns")
    _raises(ARG, lambda: s.spec_begin(3, [word("NA")], [0], True))
    s.spec_begin(3, [word("NGN")], [6], False)  # (G>A is a type of its own without folding)
    s.spec_end()
    # the same pattern under two types of one REF is fine: different slots
    s.spec_begin(3, [word("NAN"), word("NAN")], [0, 1], True)
    try:
        _raises(ARG, lambda: s.spec_sites(seq, [1, 2], b"AN"), "site 1 has an ALT byte")
        _raises(ARG, lambda: s.spec_sites(seq, [50], b"A"), "site 0")
        _raises(ARG, lambda: s.spec_regions(seq, [(5, 4)]))
        _raises(ARG, lambda: s.spec_track(seq, 0, 51))
        _raises(STATE, lambda: s.spec_begin(3, [word("NAN")], [0], True))
    finally:
        s.spec_end()
    for call in (lambda: s.spec_regions(seq, [(0, 1)]), lambda: s.spec_track(seq), lambda: s.spec_sites(seq, [1], b"A"),
                 lambda: s.spec_end()):
        _raises(STATE, call)
    # typed and plain site calls in the wrong kind of session
    s.seq_begin_typed(3, True)
    try:
        _raises(STATE, lambda: s.seq_sites(seq, [1]))
        _raises(STATE, lambda: s.seq_end())
        _raises(STATE, lambda: s.seq_begin(3, True))
        _raises(ARG, lambda: s.seq_sites_typed(seq, [1], b"x"), "ALT byte")
        s.seq_scan(seq)
    finally:
        s.seq_end_typed()
    s.seq_begin(3, True)
    try:
        _raises(STATE, lambda: s.seq_sites_typed(seq, [1], b"A"))
        _raises(STATE, lambda: s.seq_end_typed())
    finally:
        s.seq_end()
    _raises(ARG, lambda: s.seq_begin_typed(2, True))
    with pytest.raises(ValueError):
        s.spec_begin(3, [word("NAN")], [0, 1], True)


def test_types_and_model_file(tmp_path):
    assert spectrum.TYPES(True) == ["A>C", "A>G", "A>T", "C>A", "C>G", "C>T"] == R.types(True)
    assert spectrum.TYPES(False) == R.ALL_TYPES and len(R.ALL_TYPES) == 12
    assert spectrum.type_id("G>A", True) == 5 and spectrum.type_id("g>a", False) == 6 and spectrum.type_id("T>G", False) == 11
    for t, kind in enumerate(R.ALL_TYPES):
        assert spectrum.type_id(kind, False) == t == 3 * "ACGT".index(kind[0]) + R.slot(kind[0], kind[2])
        assert spectrum.slot_of(kind[0], kind[2]) == t % 3
    with pytest.raises(ValueError):
        spectrum.type_id("A>A")
    parts = {"C>T": (["NCG", "NCH"], [(5, 100), (1, 300)], [0.1, 1 / 3]), "A>G": (["NAN"], [(2, 50)], [1e-9])}
    m = spectrum.Model.from_partitions(parts)
    assert m.types == ["A>G", "C>T"] and m.names == ["NAN", "NCG", "NCH"] and m.ptype.tolist() == [1, 5, 5] and m.k == 3
    m.write(tmp_path / "m.txt")
    text = open(tmp_path / "m.txt").read()
    assert text == "type pattern p_neg p_pos p_rate\nA>G NAN 50 2 1e-09\nC>T NCG 100 5 0.1\nC>T NCH 300 1 0.3333333333333333\n"
    back = spectrum.Model.read(tmp_path / "m.txt")
    assert back.names == m.names and back.rates.tobytes() == m.rates.tobytes() and back.counts == m.counts
    assert back.ptype.tolist() == m.ptype.tolist() and back.folded
    with pytest.raises(ValueError):
        spectrum.Model.read(io.StringIO("pattern p_neg p_pos p_rate\nNAN 1 1 0.5\n"))
    with pytest.raises(ValueError):
        spectrum.Model(["NCN", "NAN"], [3, 0], [0.1, 0.2])


def test_api_functions_and_batching():
    rng = np.random.RandomState(5)
    names, ptype, rates = _model(9, 5, True, 6, 8)
    model = spectrum.Model(names, ptype, rates)
    contigs = [("a", R.random_seq(rng, 900, lower=0.2, invalid=0.01)), ("b", R.random_seq(rng, 333)), ("c", R.random_seq(rng, 50))]
    regions = {"a": [(0, 900), (100, 400), (350, 800), (5, 5)], "b": [(0, 333), (300, 333)]}
    full = spectrum.region_rates(contigs, model, regions, want_hist=True, host=True)
    small = spectrum.region_rates(contigs, model, regions, want_hist=True, host=True, budget=len(names) + 1)
    assert sorted(full) == ["a", "b"]
    for name, seq in contigs[:2]:
        rh, ro, re = R.regions(seq, names, ptype, True, regions[name], rates)
        for got in (full[name], small[name]):
            assert np.array_equal(got[0], rh) and np.array_equal(got[1], ro) and got[2].tobytes() == re.tobytes()
    assert spectrum.region_rates(contigs, model, regions, host=True)["a"][0] is None
    trk = spectrum.track(contigs, model, host=True)
    assert np.array_equal(trk["c"], R.track(contigs[2][1], names, ptype, True))
    assert np.array_equal(spectrum.track(contigs[0][1], model, host=True, begin=7, end=99), trk["a"][:, 7:99])
    pos = rng.randint(0, 333, size=60)
    alts = _alts(rng, contigs[1][1], pos)
    got = spectrum.site_rates(contigs, model, {"b": (pos, alts)}, host=True)
    assert np.array_equal(got["b"], R.sites(contigs[1][1], names, ptype, True, pos, alts))
    assert {-3} < set(got["b"].tolist())
    tables = spectrum.count_tables(contigs, 5, sites={"b": (pos, alts)}, host=True)
    one = C.count_table(contigs, 5, host=True)
    assert sum(len(t) for t in tables.values()) == 3 * len(one)  # (a k-mer is a row of its REF's three types)
    assert sum(int(t.M.sum()) for t in tables.values()) == int((got["b"] > -2).sum())


def _write_inputs(tmp_path, rng, fmt):
    contigs = [("chr1", R.random_seq(rng, 1500, lower=0.3, invalid=0.004)), ("chr2", R.random_seq(rng, 700))]
    genome = str(tmp_path / ("g.fa" if fmt == "fasta" else "g.2bit"))
    if fmt == "fasta":
        R.write_fasta(genome, contigs)
    else:
        R.write_2bit(genome, contigs)
        contigs = [(n, np.where(np.isin(s & 0xDF, list(b"ACGT")), s, ord("N")).astype(np.uint8)) for n, s in contigs]
    rows = []
    for name, seq in contigs:
        for p in rng.randint(0, seq.shape[0], size=400).tolist() + [0, 0, seq.shape[0] - 1]:
            ref = chr(seq[p]).upper()
            if ref in "ACGT":
                alt = "ACGT"[("ACGT".index(ref) + 1 + rng.randint(3)) % 4]
                rows.append((name, p + 1, ref if rng.randint(20) else "ACGT"[("ACGT".index(ref) + 1) % 4], alt))
    rows += [("chr1", 5000, "A", "C"), ("chrX", 1, "A", "C"), ("chr1", 7, "AT", "A"), ("chr2", 9, "N", "A"),
             ("chr1", 8, "g", "G"), ("chr2", 30, "T", "T")]
    order = rng.permutation(len(rows))
    rows = [rows[i] for i in order]
    with open(tmp_path / "m.txt", "w") as f:
        f.write("#CHROM POS REF ALT\n" + "".join(f"{c} {p} {r} {a}\n" for c, p, r, a in rows))
    return genome, contigs, rows


@pytest.mark.parametrize("fmt", ["fasta", "2bit"])
def test_command_line(tmp_path, capsys, fmt):
    rng = np.random.RandomState(3)
    genome, contigs, rows = _write_inputs(tmp_path, rng, fmt)
    sites = str(tmp_path / "m.txt")
    k = 5
    # count: byte-identical to six kmerpapa-count runs
    assert spectrum.main(["count", genome, sites, "-k", "5", "-o", str(tmp_path / "c")], host=True) == 0
    err = capsys.readouterr().err
    same = sum(len(r) == 1 and r.upper() in "ACGT" and r.upper() == a.upper() for _, _, r, a in rows)
    assert same >= 2 and f"alt_equals_ref={same}\n" in err and f"not_snv={same + 2}\n" in err and "ref_mismatch=" in err and "sites_skipped=" in err
    assert C.main(["background", genome, "-k", "5", "-o", str(tmp_path / "bg.txt"), "--verbosity", "0"], host=True) == 0
    assert open(tmp_path / "c.background.txt").read() == open(tmp_path / "bg.txt").read()
    for kind in R.types(True):
        one = str(tmp_path / "one.txt")
        assert C.main(["snv", genome, sites, "--type", kind, "--radius", "2", "-o", one, "--verbosity", "0"], host=True) == 0
        assert open(tmp_path / f"c.{kind[0]}_{kind[2]}.txt").read() == open(one).read() != ""
    # join: a model of every type, and its round trip
    names, ptype, rates = _model(21, k, True, 6, 7, empty=4)
    by_type = {}
    for x, t, r in zip(names, ptype, rates.tolist()):
        by_type.setdefault(t, []).append((x, r))
    argv = []
    for t, part in by_type.items():
        path = tmp_path / f"p{t}.txt"
        with open(path, "w") as f:
            if t % 2:
                f.write("pattern p_neg p_pos p_rate\n" + "".join(f"{x} 10 1 {r!r}\n" for x, r in part))
            else:
                f.write("context c_neg c_pos c_rate pattern p_neg p_pos p_rate\n" +
                        "".join(f"AAAAA 1 1 0.5 {x} 10 1 {r!r}\n" * 2 for x, r in part))
        argv += ["--type", f"{R.ALL_TYPES[t].lower()}={path}"]
    model_file = str(tmp_path / "model.txt")
    assert spectrum.main(["join", "-o", model_file] + argv) == 0
    model = spectrum.Model.read(model_file)
    assert model.names == names and model.ptype.tolist() == ptype and model.rates.tobytes() == rates.tobytes()
    assert model.types == [R.ALL_TYPES[t] for t in sorted(by_type)] and len(model.types) == 5
    # regions, with --observed over overlapping regions
    bed = [("chr1", 100, 900, "geneA"), ("chr2", 0, 10, "geneB"), ("chr1", 800, 1500, "geneC"), ("chrX", 1, 2, "geneD"),
           ("chr1", 0, 1500, "all"), ("chr2", 0, 700, "all2")]
    with open(tmp_path / "r.bed", "w") as f:
        f.write("track name=x\n" + "".join(f"{c}\t{b}\t{e}\t{x}\n" for c, b, e, x in bed))
    out = str(tmp_path / "out.txt")
    base = ["--model", model_file, "--verbosity", "0"]
    assert spectrum.main(["regions", genome, "--bed", str(tmp_path / "r.bed"), "--observed", sites, "-o", out] + base,
                         host=True) == 0
    lines = open(out).read().splitlines()
    kinds = model.types
    assert lines[0].split() == (["#chrom", "start", "end", "name", "valid", "invalid", "exp_total"] +
                                [f"exp_{x}" for x in kinds] + ["obs_total"] + [f"obs_{x}" for x in kinds])
    seqs = dict(contigs)
    accepted = 0
    for line, (c, b, e, label) in zip(lines[1:], bed):
        tok = line.split()
        assert tok[:4] == [c, str(b), str(e), label]
        if c not in seqs:
            assert tok[4:6] == ["0", "0"] and set(tok[6:6 + 1 + len(kinds)]) == {"0.0"}
            continue
        _, ro, re = R.regions(seqs[c], names, ptype, True, [(b, e)], rates)
        assert tok[4:6] == [str(e - b - int(ro[0, 3])), str(int(ro[0, 3]))]
        total = 0.0
        for x in kinds:
            total = total + float(re[0, R.ALL_TYPES.index(x)])
        assert tok[6] == repr(total) and tok[7:7 + len(kinds)] == [repr(float(re[0, R.ALL_TYPES.index(x)])) for x in kinds]
        obs = dict.fromkeys(kinds, 0)
        for cc, p, r, a in rows:
            if cc == c and b <= p - 1 < e and len(r) == 1 and r in "ACGT" and p <= len(seqs[c]) and \
                    chr(seqs[c][p - 1]).upper() == r and r != a:
                if r in "GT":
                    r, a = R.COMPLEMENT[r], R.COMPLEMENT[a]
                if r + ">" + a in obs:
                    obs[r + ">" + a] += 1
        assert tok[7 + len(kinds):] == [str(sum(obs.values()))] + [str(obs[x]) for x in kinds]
        accepted += sum(obs.values()) if label in ("all", "all2") else 0
    assert accepted > 500
    # track: the sum over the REF's types, and one type
    for extra, kind in (([], None), (["--type", "G>A"], "C>T")):
        assert spectrum.main(["track", genome, "-o", out] + extra + base, host=True) == 0
        want = ""
        for name, seq in contigs:
            pid = R.track(seq, names, ptype, True)
            want += R.bedgraph(name, 0, R.track_values(seq, names, ptype, rates, True, pid, 0, kind))
        assert open(out).read() == want != ""
    assert spectrum.main(["track", genome, "--bed", str(tmp_path / "r.bed"), "-o", out] + base, host=True) == 0
    pid = R.track(seqs["chr2"], names, ptype, True)
    assert R.bedgraph("chr2", 0, R.track_values(seqs["chr2"], names, ptype, rates, True, pid, 0)) in open(out).read()
    # sites
    assert spectrum.main(["sites", genome, sites, "-o", out] + base, host=True) == 0
    got = open(out).read().splitlines()
    snv = [(c, p, r, a) for c, p, r, a in rows if len(r) == 1 and r in "ACGT" and a in "ACGT" and r.upper() != a.upper()]
    assert len(got) == len(snv)
    hits = 0
    for line, (c, p, r, a) in zip(got, snv):
        tail = "NA NA NA"
        if c in seqs and p <= len(seqs[c]) and chr(seqs[c][p - 1]).upper() == r:
            j = int(R.sites(seqs[c], names, ptype, True, [p - 1], [a])[0])
            if j >= 0:
                tail = f"{R.ALL_TYPES[ptype[j]]} {names[j]} {float(rates[j])!r}"
                hits += 1
        assert line == f"{c} {p} {r} {a} {tail}"
    assert hits > 300


def test_command_line_errors(tmp_path, capsys):
    rng = np.random.RandomState(8)
    genome, contigs, rows = _write_inputs(tmp_path, rng, "fasta")
    with open(tmp_path / "r.bed", "w") as f:
        f.write("chr1 0 10\n")

    def run(argv):
        rc = spectrum.main(argv, host=True)
        return rc, capsys.readouterr().err

    def model(text):
        with open(tmp_path / "model.txt", "w") as f:
            f.write("type pattern p_neg p_pos p_rate\n" + text)
        return ["--model", str(tmp_path / "model.txt")]

    reg = ["regions", genome, "--bed", str(tmp_path / "r.bed")]
    rc, err = run(reg + model("C>T NCN 1 1 0.5\nC>T ACG 1 1 0.5\n"))
    assert rc == 1 and "kmerpapa-spectrum: a type's patterns are not a partition: 1 pairs" in err
    for text in ("C>T NAN 1 1 0.5\n", "C>T NCN 1 1 0.5\nA>C NAN 1 1 0.5\n", "C>C NCN 1 1 0.5\n", "C>T NCN 1 1\n", "",
                 "G>A NGN 1 1 0.5\n", "C>T NC 1 1 0.5\n"):
        rc, err = run(reg + model(text))
        assert rc == 2 and err.startswith("kmerpapa-spectrum: input error: "), text
    assert run(reg + model("G>A NGN 1 1 0.5\n") + ["--no-fold"])[0] == 0
    ok = model("C>T NCN 1 1 0.5\n")
    assert run(["regions", str(tmp_path / "none.fa"), "--bed", str(tmp_path / "r.bed")] + ok)[0] == 2
    assert run(["track", genome, "--type", "A>C"] + ok)[0] == 2
    assert run(["count", genome, str(tmp_path / "m.txt"), "-k", "4", "-o", str(tmp_path / "c")])[0] == 2
    assert run(["count", genome, str(tmp_path / "m.txt"), "-k", "16", "--no-fold", "-o", str(tmp_path / "c")])[0] == 2
    assert run(["join", "--type", "C>T", "-o", str(tmp_path / "x")])[0] == 2
    assert run(["join", "--type", f"C>T={tmp_path / 'model.txt'}", "-o", str(tmp_path / "x")])[0] == 2
    with open(tmp_path / "p.txt", "w") as f:
        f.write("pattern p_neg p_pos p_rate\nNAN 1 1 0.5\n")
    rc, err = run(["join", "--type", f"C>T={tmp_path / 'p.txt'}", "-o", str(tmp_path / "x")])
    assert rc == 2 and "REF base in the centre" in err
    with open(tmp_path / "bad.txt", "w") as f:
        f.write("chr1 x A C\n")
    assert run(["sites", genome, str(tmp_path / "bad.txt")] + ok)[0] == 2


def test_patterns_in_any_order():
    """The pattern list need not be grouped by type: ``expected`` adds a type's patterns in
    ascending index order wherever they stand."""
    rng = np.random.RandomState(77)
    names, ptype, rates = _model(5, 5, True, 6, 9)
    order = rng.permutation(len(names))
    names, ptype, rates = [names[i] for i in order], [ptype[i] for i in order], rates[order]
    assert any(a > b for a, b in zip(ptype, ptype[1:]))
    seq = R.random_seq(rng, 600, lower=0.2, invalid=0.01)
    regs = _regions(600)
    hist, other, exp, _, _, _ = engine.spec_host(5, [word(x) for x in names], ptype, True, seq, regs, rates)
    rh, ro, re = R.regions(seq, names, ptype, True, regs.tolist(), rates)
    assert np.array_equal(hist, rh) and np.array_equal(other, ro) and exp.tobytes() == re.tobytes()
