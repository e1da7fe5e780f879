"""The class order of the block list (kp_plan.h build_plan, kp_core.h kp_block_slot): inside
a high level the blocks go by slab (the digits of the slow positions), then by the digit
levels of the fast positions (the class), then by the fast digits without siblings, then by
those with siblings, level 1 first, the highest level fastest.  KP_BLOCK_CLASS=1 (the default) selects it,
0 the plain mixed-radix order.  Host code, no GPU.

The key is restated here with numpy from pattern_utils' code tables (it shares no code with
kp_plan.h) and must give the host's list entry for entry."""
import hashlib

import numpy as np
import pytest

from kmerpapa_amd import engine
from kmerpapa_amd import pattern_utils as pu

SMALL = [("NNNNN", 16), ("NNMNNN", 16), ("RYSWKMBDHVN", 16)]
LATTICES = SMALL + [("NNNNNNN", 16), ("NNNNMNNNN", 4096)]
KNOBS = ("KP_BLOCK_CLASS", "KP_BLOCK_PERM", "KP_BLOCK_TILE", "KP_BLOCK_ORDER", "KP_NT_SLOW")

# sha256 of the NNNNN / max_block 16 list (uint32, little endian) of the commit before the
# class order: what KP_BLOCK_CLASS=0 has to give
PARENT_NNNNN_SHA256 = "c674931f471a288a8d6d19a249a5cff528135b9902b7460d286bd7d4bf12ce6b"


@pytest.fixture
def knobs(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    return monkeypatch


class Lattice:
    """The blocked lattice of a general pattern: low positions as many as fit max_block,
    the others high; block h = mixed radix over the high digits, the first high position
    least significant."""

    def __init__(self, gen_pat, max_block, perm=None, slow=3):
        radix = [len(pu.perm_code[g]) for g in gen_pat]
        t, cells = 0, 1
        while t < len(gen_pat) and t < 8 and cells * radix[t] <= max_block:
            cells *= radix[t]
            t += 1
        if t == 0:
            t = 1
        self.high = gen_pat[t:]
        self.kh = len(self.high)
        self.radix = radix[t:]
        self.nblocks = int(np.prod(self.radix, dtype=np.int64)) if self.kh else 1
        self.place = [int(np.prod(self.radix[:i], dtype=np.int64)) for i in range(self.kh)]
        # per position and digit: level, split pairs, has siblings, children (digit pairs)
        self.lev, self.sib, self.pairs = [], [], []
        for g in self.high:
            letters = pu.perm_code[g]
            lev = [pu.code_level[x] for x in letters]
            self.lev.append(np.array(lev))
            self.sib.append(np.array([pu.n_complements_of[x] > 0 and lev.count(pu.code_level[x]) > 1
                                      for x in letters]))
            self.pairs.append([[(letters.index(a), letters.index(b)) for a, b in pu.complements.get(x, ())]
                               for x in letters])
        if perm is None:  # largest radix fastest, later positions before earlier ones
            perm = sorted(range(self.kh - 1, -1, -1), key=lambda i: -self.radix[i])
        else:
            perm = list(perm) + [i for i in range(self.kh - 1, -1, -1) if i not in perm]
        self.perm = perm
        # the slow positions: from the slowest end of perm until `slow` of them have split pairs
        nfast = self.kh
        while nfast > 0 and slow > 0:
            nfast -= 1
            slow -= self.radix[perm[nfast]] > 1
        self.nfast = nfast
        h = np.arange(self.nblocks, dtype=np.int64)
        self.dig = [(h // self.place[i]) % self.radix[i] for i in range(self.kh)]
        self.level = sum((self.lev[i][self.dig[i]] for i in range(self.kh)), np.zeros(self.nblocks, dtype=np.int64))

    def _pack(self, positions, bits, value, where=None):
        """One integer per block: value(i) of the given positions, the first most significant;
        positions where `where(i)` is false leave no digit."""
        w = np.zeros(self.nblocks, dtype=np.int64)
        for i in positions:
            v = value(i)
            if where is None:
                w = (w << bits) | v
            else:
                m = where(i)
                w = np.where(m, (w << bits) | v, w)
        return w

    def class_order(self):
        """The list under the key of the class order."""
        slowest_first = self.perm[::-1]
        slow, fast = slowest_first[:self.kh - self.nfast], slowest_first[self.kh - self.nfast:]
        flev = {i: self.lev[i][self.dig[i]] for i in fast}
        fsib = {i: self.sib[i][self.dig[i]] for i in fast}
        keys = [self.level,
                self._pack(slow, 4, lambda i: self.dig[i]),
                self._pack(fast, 2, lambda i: flev[i]),
                self._pack(fast, 4, lambda i: self.dig[i], lambda i: ~fsib[i])]
        for lvl in (1, 2, 3):
            keys.append(self._pack(fast, 4, lambda i: self.dig[i], lambda i: fsib[i] & (flev[i] == lvl)))
        return np.lexsort(keys[::-1]).astype(np.uint32)

    def plain_order(self):
        """The list of the plain order: every level in the mixed-radix order of perm."""
        return np.lexsort([self.dig[i] for i in self.perm] + [self.level]).astype(np.uint32)


def _list(gen_pat, max_block):
    hlist, hoff = engine.block_list_host(gen_pat, max_block)
    return hlist, hoff.astype(np.int64)


@pytest.mark.parametrize("env", [{}, {"KP_BLOCK_CLASS": "1"}, {"KP_BLOCK_CLASS": "0"},
                                 {"KP_BLOCK_CLASS": "1", "KP_BLOCK_PERM": "3-0-1"}], ids=["default", "on", "off", "perm"])
@pytest.mark.parametrize("gen_pat,max_block", LATTICES)
def test_closed_form_matches_host_sort(knobs, gen_pat, max_block, env):
    for k, v in env.items():
        knobs.setenv(k, v)
    assert engine.block_order_check(gen_pat, max_block) == 0


@pytest.mark.parametrize("gen_pat,max_block", SMALL)
def test_host_list_is_the_restated_key(knobs, gen_pat, max_block):
    knobs.setenv("KP_BLOCK_CLASS", "1")
    hlist, _ = _list(gen_pat, max_block)
    L = Lattice(gen_pat, max_block)
    assert np.array_equal(hlist, L.class_order())
    # with one fast position the key is the plain order (a level's digits ascending); with
    # more the list has to differ from it
    assert np.array_equal(hlist, L.plain_order()) == (L.nfast < 2)


@pytest.mark.parametrize("gen_pat,max_block", SMALL)
def test_host_list_under_explicit_permutation_and_slow_count(knobs, gen_pat, max_block):
    """Slab and fast sets follow KP_BLOCK_PERM and KP_NT_SLOW."""
    knobs.setenv("KP_BLOCK_CLASS", "1")
    knobs.setenv("KP_BLOCK_PERM", "2-0-3")
    knobs.setenv("KP_NT_SLOW", "2")
    hlist, _ = _list(gen_pat, max_block)
    assert np.array_equal(hlist, Lattice(gen_pat, max_block, perm=[2, 0, 3], slow=2).class_order())


@pytest.mark.parametrize("gen_pat,max_block", LATTICES)
def test_list_is_a_permutation_with_the_levels_in_their_ranges(knobs, gen_pat, max_block):
    knobs.setenv("KP_BLOCK_CLASS", "1")
    hlist, hoff = _list(gen_pat, max_block)
    L = Lattice(gen_pat, max_block)
    assert hlist.size == L.nblocks and hoff[0] == 0 and hoff[-1] == L.nblocks
    assert np.array_equal(np.sort(hlist), np.arange(L.nblocks, dtype=np.uint32))
    assert np.array_equal(np.diff(hoff), np.bincount(L.level, minlength=hoff.size - 1))
    for s in range(hoff.size - 1):
        assert np.all(L.level[hlist[hoff[s]:hoff[s + 1]]] == s)


def test_default_is_the_class_order(knobs):
    assert np.array_equal(_list("NNMNNN", 16)[0], Lattice("NNMNNN", 16).class_order())


def test_switch_off_gives_the_parent_list(knobs):
    knobs.setenv("KP_BLOCK_CLASS", "0")
    hlist, _ = _list("NNNNN", 16)
    assert hashlib.sha256(hlist.astype("<u4").tobytes()).hexdigest() == PARENT_NNNNN_SHA256
    assert np.array_equal(hlist, Lattice("NNNNN", 16).plain_order())
    for gen_pat, max_block in SMALL[1:]:
        assert np.array_equal(_list(gen_pat, max_block)[0], Lattice(gen_pat, max_block).plain_order())


@pytest.mark.parametrize("gen_pat,max_block", [("NNN", 16), ("NNNN", 16), ("NNMN", 16), ("ANNNA", 16)])
def test_no_fast_position_keeps_the_plain_list(knobs, gen_pat, max_block):
    """No more high positions (with split pairs) than slow ones: exactly the plain list."""
    knobs.setenv("KP_BLOCK_CLASS", "1")
    new, _ = _list(gen_pat, max_block)
    knobs.setenv("KP_BLOCK_CLASS", "0")
    old, _ = _list(gen_pat, max_block)
    assert np.array_equal(new, old)
    assert np.array_equal(new, Lattice(gen_pat, max_block).plain_order())


@pytest.mark.parametrize("gen_pat,max_block", SMALL)
def test_children_lie_in_earlier_levels(knobs, gen_pat, max_block):
    """What the sweep relies on: a block's split children sit in the slot range of an
    earlier level (launch)."""
    knobs.setenv("KP_BLOCK_CLASS", "1")
    hlist, hoff = _list(gen_pat, max_block)
    L = Lattice(gen_pat, max_block)
    slot = np.empty(L.nblocks, dtype=np.int64)
    slot[hlist] = np.arange(L.nblocks)
    h = np.arange(L.nblocks, dtype=np.int64)
    level_start = hoff[L.level]
    checked = 0
    for i in range(L.kh):
        for d, pairs in enumerate(L.pairs[i]):
            mine = h[L.dig[i] == d]
            for pair in pairs:
                for c in pair:
                    assert c < d
                    child = mine - (d - c) * L.place[i]
                    assert np.all(slot[child] < level_start[mine])
                    checked += mine.size
    assert checked > 0
