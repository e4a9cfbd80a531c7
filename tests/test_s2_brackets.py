"""CPU: the documents of tests/s2_brackets.py are what they claim.  The oracle accepts the valid ones and rejects the others,
the mirror's two statements of the matcher (from the answer, and window by window on the level arrays) agree with each other
and with a plain scan, and over the whole set every part of k_br_match / wave_psv_tree is reached at every edge that can
occur.  tests/test_gpu_brackets.py runs the same documents on the device."""
import collections
import functools

import numpy as np
import pytest

import oracle_lib as O
import s2_brackets as B

ALL_EDGES = ("c_lane0", "c_lane63", "a_lane0", "a_lane63", "hit_first", "hit_last", "idx_mult64")
# The edges a class can have.  What is left out can not occur in any document:
#   * between an answer a and the bracket c that asks there lie one open bracket and balanced pairs, so c - a is even, and
#     with no answer (a = -1) c is odd: a question without an answer never sits in lane 0;
#   * own_group: the answer is a lower lane of the same group (c is not lane 0, a is not lane 63) and there is no window;
#   * group_in_front has no climb, none_g0 / none_idx0 end in front of the first window;
#   * none_top can not occur at all (s2_brackets docstring).
REQUIRED = {
    "own_group": ("c_lane63", "a_lane0"),
    "group_in_front": ("c_lane0", "c_lane63", "a_lane0", "a_lane63", "hit_first", "hit_last"),
    "tree(1)": ALL_EDGES,
    "tree(2)": ALL_EDGES,
    "tree(3)": ALL_EDGES,
    "none_g0": ("c_lane63",),
    "none_idx0": ("c_lane63",),
    "none_hb0": ("c_lane63", "idx_mult64"),
}


@functools.lru_cache(maxsize=None)
def docs():
    return B.valid_docs()


@functools.lru_cache(maxsize=None)
def view(name):
    doc, nd = docs()[name]
    ok, pos = O.stage1(doc, nd)
    assert ok, name
    return B.View(doc, pos)


@functools.lru_cache(maxsize=None)
def cover(name):
    return B.coverage(view(name))


def test_valid_documents_parse_and_the_mirror_knows_their_tape_offsets():
    for name, (doc, nd) in docs().items():
        ref = O.parse(doc, ndjson=nd)
        assert ref.rc == 0, name
        v = view(name)
        tags = (ref.tape[v.off] >> np.uint64(56)).astype(np.uint8)
        assert np.array_equal(tags, v.ch), name  # every bracket's word lies where the mirror says


def test_error_documents_are_rejected_and_their_repaired_twins_are_not():
    errs = B.error_docs()
    assert len(errs) >= 16
    for name, doc in errs.items():
        assert O.parse(doc).rc != 0, name
    # the defect is the only one: the same call without it gives a valid document
    assert O.parse(B.far_pair_doc(13000, (63,), ("obj",))).rc == 0
    assert O.parse(B.far_pair_doc(400, (10,), ("arr",), seam_behind_opener=True)).rc == 0
    assert O.parse(B.far_pair_doc(9000, ())).rc == 0


def test_count_documents_hold_exactly_the_brackets_asked_for():
    for n in B.COUNTS:
        doc, valid = B.count_doc(n)
        assert valid == (n % 2 == 0)
        ok, pos = O.stage1(doc)
        v = B.View(doc, pos)
        assert v.n == n, (n, v.n)
        assert len(v.levels()) == 1 + sum(n > 64 ** k for k in (1, 2, 3))
        if valid:  # one outermost pair: the close asks across everything
            assert v.depth[0] == 1 and v.depth[-1] == 0 and (v.depth[:-1] >= 1).all()
    for n in B.COUNTS:  # the valid neighbour of an odd count has the same level sizes
        if n % 2:
            assert [-(-n // 64 ** k) for k in (1, 2, 3)] == [-(-(n + 1) // 64 ** k) for k in (1, 2, 3)]
            assert view("count_%d" % (n + 1)).n == n + 1


def test_host_and_device_level_documents():
    a, b = view("levels_host4_device3"), view("levels_both4")
    assert a.n_tokens > 64 ** 3 and 4096 < a.n <= 64 ** 3  # the launcher sizes four levels, the device builds three
    assert len(a.levels()) == 3
    assert b.n > 64 ** 3 and len(b.levels()) == 4


def _sample(v, live, k=250):
    c = np.flatnonzero(live)
    if len(c) <= 2 * k:
        return c
    rnd = np.random.RandomState(len(c))
    return np.unique(np.concatenate([c[:40], c[-k:], rnd.choice(c, k, replace=False)]))


def test_the_mirror_agrees_with_a_scan_and_with_the_walk_over_the_level_arrays():
    for name in docs():
        v = view(name)
        a_all = v.answers()
        live = v.live(a_all)
        c, a, cls, level, first, last, mult = B.classify(v, a_all)
        assert np.array_equal(c, np.flatnonzero(live))
        at = {int(x): i for i, x in enumerate(c)}
        lev = v.levels()
        for x in _sample(v, live):
            x = int(x)
            i = at[x]
            assert v.answer_by_scan(x) == a[i], (name, x)
            w = B.walk(v, lev, x)
            assert (w.cls, w.a, w.level, w.hit_first, w.hit_last, w.idx_mult64) == \
                (B.CLASSES[cls[i]], a[i], level[i], first[i], last[i], mult[i]), (name, x, w)
        # brackets that are not live: q < 0, or the answer in the tile
        rnd = np.random.RandomState(v.n)
        for x in rnd.choice(v.n, min(v.n, 60), replace=False):
            if not live[x] and v.q[x] >= 0:
                s = v.answer_by_scan(int(x))
                assert s == a_all[x] and s >= 0 and v.tile[s] == v.tile[x], (name, x)


def test_every_class_is_reached_at_every_edge():
    total = collections.Counter()
    for name in docs():
        total.update(cover(name))
    missing = [(cls, e) for cls, edges in REQUIRED.items() for e in ("",) + tuple(edges) if total[(cls, e)] == 0]
    assert not missing, missing
    assert total[("none_top", "")] == 0
    for cls in B.CLASSES:  # nothing the table does not know about
        if cls not in REQUIRED:
            assert total[(cls, "")] == 0, cls


def test_excursion_answers_are_alone_in_their_windows():
    """every level's entry of the answer is the only one in its window of 64 that is as low as the question -- and it is
    found through level 2 (level 3 in the large document), in every quarter of a level-2 entry"""
    quarters = set()
    for name in docs():
        if not name.startswith("excursion"):
            continue
        v = view(name)
        a_all = v.answers()
        c, a, cls, level, first, last, mult = B.classify(v, a_all)
        top = 3 if name == "excursion3" else 2
        far = np.flatnonzero(cls == B.CLASSES.index("tree(%d)" % top))
        x = int(a[far].max())  # the close bracket of the excursion
        far = far[a[far] == x]
        assert len(far) > 60 and v.is_close[x], name
        q = int(v.q[c[far[0]]])
        lev = v.levels()
        for L in range(0, top):
            e = x >> (6 * L)
            w = lev[L][(e >> 6) << 6:((e >> 6) << 6) + 64]
            assert (w <= q).sum() == 1 and lev[L][e] <= q, (name, L)
        quarters.add((x >> 10) & 3)
        if top == 3:
            assert x >> 18 == 1  # not the first entry of level 3: what k_min_upper wrote there decides
    assert quarters == {0, 1, 2, 3}


def test_staircase_has_waves_of_64_distinct_live_questions():
    v = view("staircase")
    a = v.answers()
    live = v.live(a)
    full = [g for g in range(v.n // 64)
            if live[g * 64:g * 64 + 64].all() and v.is_close[g * 64:g * 64 + 64].all() and len(set(v.q[g * 64:g * 64 + 64])) == 64]
    assert len(full) >= 1
    ans = np.concatenate([a[g * 64:g * 64 + 64] for g in full])
    assert (ans >= 0).all()
    assert len(set(ans >> 6)) >= 8 and len(set(ans >> 12)) >= 3 and len(set(v.tile[ans])) >= 3
    assert len(set(v.ch[ans + 1])) == 2  # arrays and objects among the partners


def test_long_records_close_through_the_matcher_at_both_parities():
    for name in ("long_records_nd",):
        cov = cover(name)
        by_edge = collections.Counter()
        for (cls, e), k in cov.items():
            by_edge[e] += k
        for e in ("root_odd", "root_even", "root_open_first", "root_open_last"):
            assert by_edge[e] > 0, (name, e)
        # the partner in the group, further in front, and nowhere (the first record)
        assert cov[("own_group", "root_odd")] and cov[("own_group", "root_even")]
        assert cov[("tree(1)", "root_odd")] + cov[("tree(1)", "root_even")] + cov[("group_in_front", "root_odd")] + cov[("group_in_front", "root_even")]
        assert cov[("none_g0", "root_even")]
        v = view(name)
        root_open = np.flatnonzero(~v.is_close & (v.depth == 1))
        tfirst = np.concatenate([[True], v.tile[1:] != v.tile[:-1]])
        tlast = np.concatenate([v.tile[1:] != v.tile[:-1], [True]])
        kinds = {(bool(tfirst[o]), bool(tlast[o])) for o in root_open}
        assert kinds == {(True, True), (True, False), (False, True), (False, False)}
        assert {int(v.off[o]) % 2 for o in root_open if tlast[o]} == {0, 1}  # long records begin at odd and even offsets
    assert O.parse(docs()["long_records_plain"][0]).rc == 0


def test_level_4_document():
    """One document of 17 million brackets (25 MB): the five-level tree, hits at level 4 at every edge."""
    doc = B.level4_doc()
    ok, pos = O.stage1(doc)
    assert ok
    v = B.View(doc, pos)
    assert v.n >= B.LEVEL4_MIN and len(v.levels()) == 5
    cov = B.coverage(v)
    missing = [e for e in ("",) + ALL_EDGES if cov[("tree(4)", e)] == 0]
    assert not missing, missing
    assert cov[("tree(3)", "")] and cov[("tree(2)", "")] and cov[("none_hb0", "")]
    # 64^4 + 1 brackets alone can not get there: the climb ends at level 3, whose only window starts at entry 0
    n = B.LEVEL4_MIN + 1
    g = (n - 1) >> 6
    idx = g - 1
    for L in (1, 2):
        idx = (((idx - 1) >> 6) << 6) >> 6
    assert ((idx - 1) >> 6) << 6 == 0
