"""Null tables per transcript by coding consequence (kp_spec_coding_null, kp_cnull.h) on the host
session (engine.HostSpec: the kernels' per-pair functions run serially) against the independent
oracle tests/coding_null_ref.py -- tests/sim_ref.py's mutation sets classed by tests/coding_ref.py,
replicate by replicate -- with the identities the header states (columns, rows, kp_spec_null's
totals), the error codes, ``spectrum.coding_null_table`` and the command line.  Every comparison is
exact equality.  No GPU."""
import ctypes

import numpy as np
import pytest

from kmerpapa_amd import engine, seqio, spectrum
from tests import coding_cases as K
from tests import coding_null_ref as N
from tests import coding_ref as C
from tests import spec_ref as R

ARG, STATE = -1, -4
SCALE = 4.0  # dense rates of 0.005 .. 0.08 become 0.02 .. 0.32: c2 up to 0.96, so every class is drawn
word = engine.pattern_word
_models = {}


def _dense(k, fold):
    """``(names, ptype, rates)`` of a random model of every type with rates 0.005 .. 0.08 (the
    dense model of tests/test_gpu_simulate.py, with the pattern names the oracle needs)."""
    if (k, fold) not in _models:
        rng = np.random.RandomState(7 * k + fold)
        names, ptype, _ = R.random_model(rng, k, fold, 6 if fold else 12, 6)
        _models[k, fold] = (names, ptype, rng.uniform(0.005, 0.08, size=len(names)))
    return _models[k, fold]


class _Session:
    def __init__(self, k, names, ptype, fold):
        self.args = (k, [word(x) for x in names], ptype, fold)

    def __enter__(self):
        self.s = engine.HostSpec()
        self.s.spec_begin(*self.args)
        return self.s

    def __exit__(self, *exc):
        self.s.spec_end()


def _same(s, got, want, stats):
    assert got.dtype == np.uint32 and got.shape == want.shape and got.tobytes() == want.tobytes()
    st = s.spec_coding_null_stats()
    assert {key: st[key] for key in stats} == stats
    assert st["stage_ms"] == st["draw_ms"] == 0.0 and st["passes"] == 1 and st["reps_per_pass"] == got.shape[1]


@pytest.mark.parametrize("k,fold", K.KSETS)
def test_host_session_equals_the_oracle_on_the_small_cases(k, fold):
    names, ptype, rates = _dense(k, fold)
    total = np.zeros(5, np.int64)
    empty_cell = False
    with _Session(k, names, ptype, fold) as s:
        for i, (name, (seq, txs)) in enumerate(sorted(K.small_cases().items())):
            for splice in K.SPLICES:
                seed, contig, first, reps = 1000 * k + 10 * i + splice, i % 3, 5 * (i % 2), 2 + i % 3
                want, stats = N.table(seq, names, ptype, rates, fold, txs, splice, seed, contig, first, reps, SCALE)
                got = s.spec_coding_null(seq, txs, rates, seed, contig, first, reps, SCALE, splice)
                _same(s, got, want, stats)
                total += want.sum(axis=(0, 1)).astype(np.int64)
                empty_cell = empty_cell or bool((want.sum(axis=2) == 0).any())
    # the comparison is one of populated tables: every class is drawn, and some cell stays empty
    assert total.min() > 0 and empty_cell, total


def test_host_session_equals_the_oracle_on_random_transcripts():
    seq, txs = K.random_case(6, 1200, 25)
    for (k, fold), splice in (((5, True), 2), ((4, False), 8)):
        names, ptype, rates = _dense(k, fold)
        want, stats = N.table(seq, names, ptype, rates, fold, txs, splice, 2 ** 63 + 9, 3, 7, 3, SCALE)
        assert want.sum(axis=(0, 1)).min() > 0 and stats["drawing"] < stats["positions"]
        # (k = 5 folded: an invalid byte in the codon also spoils the window; k = 4 reaches one base less to the right)
        assert (stats["unclassed"] > 0) == (k == 4)
        with _Session(k, names, ptype, fold) as s:
            _same(s, s.spec_coding_null(seq, txs, rates, 2 ** 63 + 9, 3, 7, 3, SCALE, splice), want, stats)


def _setup(k=5, fold=True):
    names, ptype, rates = _dense(k, fold)
    seq, txs = K.random_case(8, 2500, 30)
    return k, fold, names, ptype, rates, seq, txs


def test_replicate_batches_are_column_ranges():
    k, fold, names, ptype, rates, seq, txs = _setup()
    with _Session(k, names, ptype, fold) as s:
        whole = s.spec_coding_null(seq, txs, rates, 99, 2, 0, 7, SCALE)
        assert whole.sum() > 500
        for a, b in ((3, 4), (6, 1), (0, 2)):
            assert np.array_equal(s.spec_coding_null(seq, txs, rates, 99, 2, a, b, SCALE), whole[:, a:a + b])
        # seed, contig and scale all enter
        assert not np.array_equal(s.spec_coding_null(seq, txs, rates, 98, 2, 0, 7, SCALE), whole)
        assert not np.array_equal(s.spec_coding_null(seq, txs, rates, 99, 3, 0, 7, SCALE), whole)
        assert s.spec_coding_null(seq, txs, rates, 99, 2, 0, 7, 0.5 * SCALE).sum() < 0.7 * whole.sum()
        none = s.spec_coding_null(seq, txs, rates, 99, 2, 0, 7, 0.0)
        st = s.spec_coding_null_stats()
        assert not none.any() and st["drawing"] == st["hits"] == st["unclassed"] == 0 and st["positions"] > 1000


def test_a_row_depends_on_its_transcript_alone():
    k, fold, names, ptype, rates, seq, txs = _setup()
    with _Session(k, names, ptype, fold) as s:
        whole = s.spec_coding_null(seq, txs, rates, 5, 1, 2, 4, SCALE)
        for t in (0, 1, 7, 29):
            assert np.array_equal(s.spec_coding_null(seq, txs[t:t + 1], rates, 5, 1, 2, 4, SCALE), whole[t:t + 1])
        twice = s.spec_coding_null(seq, [txs[3], txs[3], txs[9]], rates, 5, 1, 2, 4, SCALE)
        assert np.array_equal(twice, whole[[3, 3, 9]]) and whole[3].sum() > 0
        assert np.array_equal(s.spec_coding_null(seq, txs[::-1], rates, 5, 1, 2, 4, SCALE), whole[::-1])


@pytest.mark.parametrize("k,fold", [(3, True), (4, False)])
def test_totals_are_those_of_the_null_call_over_the_same_positions(k, fold):
    """Without invalid bytes every hit has a class, so a replicate's table sums to kp_spec_null's
    column over the segments and splice intervals given as regions."""
    names, ptype, rates = _dense(k, fold)
    seq, txs = K.split_case([4, 2, 30, 9], 50)
    txs = txs + [(0, [(12, 18)]), (1, [(0, 3), (5, 8)])]
    splice = 2
    regions = []
    for _, segs in txs:
        regions += [(b, e) for b, e in segs]
        regions += [(g, g + 1) for g in C.splice_positions([(int(b), int(e)) for b, e in segs], splice)]
    with _Session(k, names, ptype, fold) as s:
        got = s.spec_coding_null(seq, txs, rates, 17, 1, 4, 6, SCALE, splice)
        st = s.spec_coding_null_stats()
        null = s.spec_null(seq, regions, rates, 17, 1, 4, 6, SCALE)
    assert st["unclassed"] == 0 and got.sum() > 100
    assert np.array_equal(got.sum(axis=(0, 2)) + st["unclassed"], null.sum(axis=0))


def test_a_hit_beside_an_invalid_byte_of_its_codon_has_no_class():
    """k = 1: the window of a base next to an N is valid, its codon is not."""
    seq, txs = K.invalid_case()
    names, ptype, rates = _dense(1, True)
    with _Session(1, names, ptype, True) as s:
        got = s.spec_coding_null(seq, txs, rates, 3, 0, 0, 8, SCALE)
        st = s.spec_coding_null_stats()
    want, stats = N.table(seq, names, ptype, rates, True, txs, 2, 3, 0, 0, 8, SCALE)
    assert got.tobytes() == want.tobytes() and st["unclassed"] == stats["unclassed"] > 0 and st["hits"] == int(got.sum())


def _raw(s, seq, txs, rates, n_reps, rep_first=0, scale=1.0, splice=2, counts=True, room=None):
    """kp_spec_coding_null itself: ``(rc, counts)`` with the output pre-filled."""
    seq = np.ascontiguousarray(seq, np.uint8)
    sb = np.array([b for _, segs in txs for b, _ in segs], np.uint64)
    se = np.array([e for _, segs in txs for _, e in segs], np.uint64)
    first = np.array(np.concatenate([[0], np.cumsum([len(segs) for _, segs in txs])]), np.uint64)
    strand = np.array([st for st, _ in txs], np.uint8)
    rates = None if rates is None else np.ascontiguousarray(rates, np.float64)
    out = np.full((len(txs) * min(n_reps, 64) * 5 if room is None else room) + 1, 0x5A5A5A5A, np.uint32)
    p = engine._ptr
    rc = engine.load().kp_spec_coding_null(s._h, p(seq), ctypes.c_uint64(seq.shape[0]), ctypes.c_uint32(0), p(sb), p(se),
                                           ctypes.c_uint64(sb.shape[0]), p(first), p(strand), ctypes.c_uint64(len(txs)),
                                           ctypes.c_uint32(splice), p(rates), ctypes.c_double(scale), ctypes.c_uint64(1),
                                           ctypes.c_uint32(rep_first), ctypes.c_uint32(n_reps), p(out) if counts else None)
    return rc, out


def _fails(s, text, *args, **kw):
    rc, out = _raw(s, *args, **kw)
    assert rc == ARG and text in engine.load().kp_last_error().decode(), engine.load().kp_last_error()
    assert np.all(out == 0x5A5A5A5A)  # (untouched)


def _raises(code, call, text=None):
    with pytest.raises(engine.KPError) as e:
        call()
    assert e.value.code == code and (text is None or text in str(e.value)), str(e.value)


def test_errors():
    seq = K.table_case()[0]
    ok_tx = [(0, [(0, 6)]), (1, [(9, 12), (20, 23)])]
    s = engine.HostSpec()
    _raises(STATE, lambda: s.spec_coding_null(seq, ok_tx, [], 1), "no session")
    # types A>C (two patterns), A>G, C>T: REF A has the types 0 and 1, REF C the type 5
    names, ptype = ["AAN", "BAN", "NAN", "NCN"], [0, 0, 1, 5]
    with _Session(3, names, ptype, True) as s:
        ok = [0.2, 0.5, 0.5, 1.0]
        rc, out = _raw(s, seq, ok_tx, ok, 3)
        assert rc == 0 and out[:30].sum() > 3 and out[30] == 0x5A5A5A5A
        # what kp_spec_coding rejects
        _fails(s, "transcript 1 hold 7 bases", seq, ok_tx[:1] + [(1, [(0, 3), (10, 14)])], ok, 3)
        _fails(s, "transcript 0 are not ascending", seq, [(0, [(0, 4), (3, 5)])], ok, 3)
        _fails(s, "is empty", seq, [(0, [(3, 3), (4, 7)])], ok, 3)
        _fails(s, "outside the contig", seq, [(0, [(190, 193)])], ok, 3)
        _fails(s, "strand that is not 0 or 1", seq, [(2, [(0, 3)])], ok, 3)
        _fails(s, "splice must be 0..8", seq, ok_tx, ok, 3, splice=9)
        # what kp_spec_null rejects
        for bad in (float("nan"), float("inf"), -1e-9):
            _fails(s, "pattern 1", seq, ok_tx, [0.1, bad, 0.1, 0.1], 3)
        for bad in (float("nan"), float("inf"), -1.0):
            _fails(s, "scale", seq, ok_tx, ok, 3, scale=bad)
        _fails(s, "REF A", seq, ok_tx, [0.2, 0.5 + 2.0 ** -52, 0.5, 1.0], 3)
        _fails(s, "REF", seq, ok_tx, ok, 3, scale=1.0000001)
        _fails(s, "no replicates", seq, ok_tx, ok, 0)
        _fails(s, "null rates", seq, ok_tx, None, 3)
        _fails(s, "2^32", seq, ok_tx, ok, 2, rep_first=2 ** 32 - 1)
        _fails(s, "2^32", seq, ok_tx, ok, 2 ** 32 - 1, rep_first=2)
        rc, out = _raw(s, seq, ok_tx, ok, 1, rep_first=2 ** 32 - 1)  # (the last replicate there is)
        assert rc == 0 and out[10] == 0x5A5A5A5A
        rc, _ = _raw(s, seq, ok_tx, ok, 3, counts=False)
        assert rc == ARG and "null counts" in engine.load().kp_last_error().decode()
        assert engine.load().kp_spec_last_coding_null(None, None) == ARG
        with pytest.raises(ValueError):
            s.spec_coding_null(seq, ok_tx, ok[:3], 1)
        with pytest.raises(ValueError):
            s.spec_coding_null(seq, ok_tx, ok, -1)
        with pytest.raises(ValueError):
            s.spec_coding_null(seq, ok_tx, ok, 1, n_reps=1 << 32)
        with pytest.raises(ValueError):
            s.spec_coding_null(seq, [(2, [(0, 3)])], ok, 1)
        _raises(ARG, lambda: s.spec_coding_null(seq, ok_tx, ok, 1, n_reps=0), "no replicates")
        _raises(ARG, lambda: s.spec_coding_null(seq, ok_tx, ok, 1, rep_first=(1 << 32) - 2, n_reps=3), "2^32")
        # nothing to do is fine, and the session is still usable after every error
        assert s.spec_coding_null(seq, [], ok, 1, n_reps=4).shape == (0, 4, 5)
        again = s.spec_coding_null(seq, ok_tx, ok, 1, n_reps=3)
        assert again.shape == (2, 3, 5) and again.tobytes() == _raw(s, seq, ok_tx, ok, 3)[1][:30].tobytes()
    _raises(STATE, lambda: s.spec_coding_null(seq, ok_tx, ok, 1), "no session")


def _transcripts(raw, contig="c"):
    return [seqio.Transcript(f"t{i}", None, contig, st, segs) for i, (st, segs) in enumerate(raw)]


def test_coding_null_table_batches_status_and_contig_ids():
    rng = np.random.RandomState(5)
    seq_a, raw_a = K.random_case(2, 1500, 12)
    seq_c, raw_c = K.random_case(3, 900, 7)
    contigs = [("a", seq_a), ("b", R.random_seq(rng, 4)), ("c", seq_c)]
    names, ptype, rates = _dense(5, True)
    model = spectrum.Model(names, ptype, rates)
    ta, tc = _transcripts(raw_a, "a"), _transcripts(raw_c, "c")
    odd = seqio.Transcript("odd", None, "a", 0, [(0, 4)])
    lost = seqio.Transcript("lost", None, "zz", 1, [(0, 6)])
    txs = tc[:3] + [odd] + ta + [lost] + tc[3:]  # contigs interleaved: rows stay in this order
    stats = {}
    whole = spectrum.coding_null_table(contigs, model, txs, 8, 7, first=2, scale=SCALE, host=True, stats=stats)
    counts, status = whole["counts"], whole["status"]
    assert counts.shape == (len(txs), 7, 5) and counts.dtype == np.uint32
    assert status.tolist() == [0] * 3 + [1] + [0] * len(ta) + [2] + [0] * (len(tc) - 3)
    assert not counts[[3, 4 + len(ta)]].any() and stats["hits"] == int(counts.sum()) > 300
    assert stats["positions"] == sum(len(w) for t in txs if t not in (odd, lost)
                                     for w in N.positions_of([(t.strand, t.segments)], 2))
    for budget in (1, 5 * 3, 5 * 7 * 2, 5 * 7 * 4 + 3):
        got = spectrum.coding_null_table(contigs, model, txs, 8, 7, first=2, scale=SCALE, host=True, budget=budget)
        assert got["counts"].tobytes() == counts.tobytes() and np.array_equal(got["status"], status)
    # the contig enters by its index in genome order, as in simulate: "c" is contig 2
    with _Session(5, names, ptype, True) as s:
        own = s.spec_coding_null(seq_c, [(t.strand, t.segments) for t in tc], rates, 8, 2, 2, 7, SCALE)
    assert np.array_equal(counts[[0, 1, 2] + list(range(5 + len(ta), len(txs)))], own)
    with pytest.raises(ValueError):
        spectrum.coding_null_table(contigs, model, txs, 8, 0, host=True)


def test_command_line(tmp_path, capsys):
    seq1, raw1 = K.random_case(11, 700, 6)
    seq2, raw2 = K.random_case(13, 500, 5)
    assert {st for st, _ in raw1} == {st for st, _ in raw2} == {0, 1}  # both strands on both contigs
    genome = str(tmp_path / "g.fa")
    R.write_fasta(genome, [("chr1", seq1), ("chr2", seq2)])
    names, ptype, rates = _dense(5, True)
    spectrum.Model(names, ptype, rates).write(str(tmp_path / "model.txt"))
    base = ["--model", str(tmp_path / "model.txt"), "--verbosity", "0"]
    txs = [seqio.Transcript(f"{c}_{i}", None, c, st, segs) for c, raw in (("chr2", raw2), ("chr1", raw1))
           for i, (st, segs) in enumerate(raw)]
    txs.insert(2, seqio.Transcript("odd", None, "chr1", 0, [(3, 8)]))
    txs.append(seqio.Transcript("lost", None, "chr9", 0, [(0, 3)]))
    bed = str(tmp_path / "cds.bed")
    with open(bed, "w") as f:
        f.write("".join(f"{t.contig} {b} {e} {t.name} 0 {'+-'[t.strand]}\n" for t in txs for b, e in t.segments))
    R_, F, seed, scale, splice = 5, 3, 77, "3.5", "3"
    # per replicate: simulate's file, and coding --observed's own obs_* columns of it
    obs = []
    for j in range(R_):
        sim = str(tmp_path / f"sim{j}.txt")
        assert spectrum.main(["simulate", genome, "--seed", str(seed), "--replicate", str(F + j), "--scale", scale, "-o", sim]
                             + base, host=True) == 0
        out = str(tmp_path / f"coding{j}.txt")
        assert spectrum.main(["coding", genome, "--cds-bed", bed, "--splice", splice, "--observed", sim, "-o", out] + base,
                             host=True) == 0
        lines = [x.split() for x in open(out).read().splitlines()]
        at = lines[0].index("obs_synonymous")
        assert lines[0][at:at + 5] == [f"obs_{c}" for c in C.CLASS_NAMES]
        obs.append([[int(v) for v in x[at:at + 5]] for x in lines[1:]])
    obs = np.array(obs).transpose(1, 0, 2)  # [transcript, replicate, class]
    assert obs.sum(axis=(0, 1)).min() > 0
    table, draws = str(tmp_path / "cnull.txt"), str(tmp_path / "draws.txt")
    args = ["coding-null", genome, "--cds-bed", bed, "--replicates", str(R_), "--seed", str(seed), "--first-replicate", str(F),
            "--scale", scale, "--splice", splice, "--draws", draws, "--observed", str(tmp_path / "sim1.txt"), "-o", table]
    assert spectrum.main(args + ["--model", str(tmp_path / "model.txt")], host=True) == 0
    err = dict(x.split("=") for x in capsys.readouterr().err.split())
    assert (err["transcripts"], err["skipped_length"], err["unknown_contig_transcripts"]) == (str(len(txs)), "1", "1")
    assert int(err["hits"]) == int(obs.sum()) and int(err["drawing"]) <= int(err["positions"]) and "unclassed" in err
    rows = [x.split() for x in open(draws).read().splitlines()]
    assert [x[:2] for x in rows] == [[t.name, c] for t in txs for c in C.CLASS_NAMES]
    got = np.array([[int(v) for v in x[2:]] for x in rows]).reshape(len(txs), 5, R_).transpose(0, 2, 1)
    assert np.array_equal(got, obs)
    lines = [x.split() for x in open(table).read().splitlines()]
    head = lines[0]
    cols = C.CLASS_NAMES + ["total", "lof"]
    want_head = ["#name", "gene", "contig", "strand", "cds_bases"] + [f"opp_{c}" for c in C.CLASS_NAMES]
    want_head += [f"exp_{c}" for c in C.CLASS_NAMES]
    for c in cols:
        want_head += [f"sim_mean_{c}", f"sim_var_{c}", f"sim_min_{c}", f"sim_max_{c}", f"obs_{c}", f"p_upper_{c}", f"p_lower_{c}"]
    assert head == want_head and len(lines) == len(txs) + 1
    # coding's own columns
    ref = [x.split() for x in open(str(tmp_path / "coding1.txt")).read().splitlines()]
    for name in want_head[:10]:
        assert [x[head.index(name)] for x in lines[1:]] == [x[ref[0].index(name)] for x in ref[1:]], name
    assert [float(x[head.index("exp_missense")]) for x in lines[1:]] == [
        float(scale) * float(x[ref[0].index("exp_missense")]) for x in ref[1:]]
    sims = [got[:, :, c] for c in range(5)] + [got.sum(axis=2), got[:, :, 2] + got[:, :, 4]]
    seen = [obs[:, 1, c] for c in range(5)] + [obs[:, 1].sum(axis=1), obs[:, 1, 2] + obs[:, 1, 4]]
    for c, one, ob in zip(cols, sims, seen):
        summary = spectrum.null_summary(one, ob)
        for i, x in enumerate(lines[1:]):
            row = dict(zip(head, x))
            assert int(row[f"obs_{c}"]) == ob[i]
            assert row[f"p_upper_{c}"] == repr((1 + int((one[i] >= ob[i]).sum())) / (R_ + 1)) == repr(summary["p_upper"][i])
            assert row[f"p_lower_{c}"] == repr((1 + int((one[i] <= ob[i]).sum())) / (R_ + 1))
            assert row[f"sim_mean_{c}"] == repr(summary["mean"][i]) and row[f"sim_var_{c}"] == repr(summary["var"][i])
            assert (int(row[f"sim_min_{c}"]), int(row[f"sim_max_{c}"])) == (one[i].min(), one[i].max())
    assert lines[3][5:15] == ["0"] * 5 + ["0.0"] * 5 and lines[3][15:22] == ["0.0", "0.0", "0", "0", "0", "1.0", "1.0"]  # (odd)
    # without --observed, on standard output, from a GTF file
    gtf = str(tmp_path / "a.gtf")
    with open(gtf, "w") as f:
        f.write("".join(f'{t.contig}\ts\tCDS\t{b + 1}\t{e}\t.\t{"+-"[t.strand]}\t0\ttranscript_id "{t.name}";\n'
                        for t in txs for b, e in t.segments))
    assert spectrum.main(["coding-null", genome, "--gtf", gtf, "--replicates", "2", "--seed", str(seed), "--scale", scale,
                          "--splice", splice, "--first-replicate", str(F + 1)] + base, host=True) == 0
    text = [x.split() for x in capsys.readouterr().out.splitlines()]
    assert len(text[0]) == 15 + 4 * 7 and text[0][-4:] == ["sim_mean_lof", "sim_var_lof", "sim_min_lof", "sim_max_lof"]
    by_name = {x[0]: x for x in text[1:]}
    for i, t in enumerate(txs):
        lof = got[i, 1:3, 2] + got[i, 1:3, 4]
        assert by_name[t.name][-4:] == [repr(float(lof.sum() / 2)), repr(float(spectrum.null_summary(lof[None])["var"][0])),
                                        str(lof.min()), str(lof.max())]
    # errors
    for bad in (["--replicates", "0"], ["--replicates", "2", "--first-replicate", str(2 ** 32 - 1)], ["--seed", "-1"],
                ["--splice", "9"], ["--scale", "100"]):
        argv = ["coding-null", genome, "--cds-bed", bed, "--replicates", "2", "--seed", "1"] + bad + base
        assert spectrum.main(argv, host=True) == 2
        assert "input error" in capsys.readouterr().err
