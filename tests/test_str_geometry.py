"""CPU checks of tests/str_geometry.py: the documents cover every (hazard, split, seam class) they claim, the oracle
gives them the verdicts they claim, the independent model agrees with the oracle's Strings.B in both copy modes, and
the host replay of sj_strings.h (csrc/host_selftest.cpp, through test_host_stage2.check) agrees with the oracle on
all of them.  Without the coverage checks the GPU tests (tests/test_gpu_string_seams.py) could pass without ever
touching a seam.

The host replay runs the per-chunk statements of sj_strings.h, the escape-by-escape general routine and the selection
scans in their sequential form.  The wave-level forms that only exist in stage2.hip (the round-robin escape list, the
ballot / carry-chain form of the selection, the walks over the unit flags, the v_perm + ds_or_b64 compaction, the
translate-where-it-landed patch) are not replayed: for those the coverage assertions here are the evidence that the
GPU tests reach every case.

Nothing is left out of the replay: the selective documents of 128 and 129 units go through it as well."""
import numpy as np
import pytest

import golden_util as GU
import oracle_lib as O
import str_geometry as S
from test_host_stage2 import L, check  # noqa: F401


def _bodies():
    return [bytes.fromhex(r["str_hex"]) for r in GU.load("strings")]


# ---- coverage of the generator -------------------------------------------------------------------------------------------
def test_rotation_covers_every_hazard_split_and_class():
    want = {(h.name, s, f) for h, s, f in S.COMBOS}
    assert len(want) == len(S.COMBOS) == 2 * sum(len(h.haz) + 1 for h in S.VALID_HAZARDS)
    assert [len(S.splits(h)) for h in S.VALID_HAZARDS if h.name in ("u_1byte", "pair")] == [7, 13]
    seen = {cls: set() for cls in S.SEAM_CLASSES}
    ends = set()
    for k in range(len(S.COMBOS)):
        lay, (eh, ef, ee) = S.rotation_layout(k)
        for cls, seam, h, s, f in lay:
            seen[cls].add((h.name, s, f))
        ends.add((eh.name, ef, ee))
    for cls in S.SEAM_CLASSES[:-1]:
        assert seen[cls] == want, cls
    assert ends == {(h.name, f, e) for h in S.VALID_HAZARDS for f in S.FORMS for e in range(4)}
    # the classes are what they say
    for cls, seam in S.rotation_seams():
        u, r = divmod(seam, S.UNIT)
        assert seam % S.CHUNK == 0 and seam < S.ROT_LENGTH
        if cls == "chunk":
            assert r != 0
        elif cls == "first":
            assert seam == S.CHUNK
        else:
            assert r == 0 and (cls == "block") == (u % S.BLOCK_UNITS == 0 and u != S.ROT_UNITS - 1)
            assert (cls == "last") == (u == (S.ROT_LENGTH - 1) // S.UNIT) and S.ROT_LENGTH % S.UNIT != 0
    assert {cls for cls, _ in S.rotation_seams()} | {"end"} == set(S.SEAM_CLASSES)


@pytest.mark.parametrize("nd", [False, True])
def test_rotation_documents_hold_the_hazard_on_the_seam(nd):
    """the bytes: hazard byte s is the first byte behind the cut, the rest of the hazard around it; the four foreign
    positions of a 'u' (the last four bytes of a chunk) occur on every class"""
    foreign = {cls: set() for cls in S.SEAM_CLASSES[:-1]}
    for d in S.rotation_docs(nd):
        lay, (eh, ef, ee) = d.info
        assert len(d.data) == S.ROT_LENGTH
        for cls, seam, h, s, f in lay:
            assert d.data[seam - s:seam - s + len(h.haz)] == h.haz, (d.name, cls, h.name, s)
            for i in range(len(h.haz) - 1):
                if h.haz[i:i + 2] == b"\\u" and 1 <= s - (i + 1) <= 4:
                    foreign[cls].add(s - (i + 1))  # the 'u' lies this many bytes in front of the cut
        tail = d.data[-(len(eh.haz) + ee + 4 + 4):]
        if eh.owns_close:
            assert tail.endswith(eh.haz + (b":1}" if ef == "key" else b"") + b" " * ee + b"]"), d.name
        else:
            assert tail.endswith(eh.haz + b"q" * ee + b'"' + (b":1}" if ef == "key" else b"") + b"]"), d.name
    assert all(v == {1, 2, 3, 4} for v in foreign.values()), foreign


@pytest.mark.parametrize("lead", [1, 63])
def test_lead_documents_put_every_combination_on_a_chunk_seam(lead):
    d = S.lead_doc(lead, False)
    _, lay = d.info
    assert {(h.name, s, f) for _, h, s, f in lay} == {(h.name, s, f) for h, s, f in S.COMBOS}
    for seam, h, s, f in lay:
        assert seam % S.CHUNK == 0 and seam % S.UNIT != 0
        at = seam - lead - s
        assert d.data[at:at + len(h.haz)] == h.haz


def test_error_documents_cover_every_hazard_split_and_class():
    seen = set()
    for d in S.error_docs():
        name, s, cls = d.info
        h = next(x for x in S.ERROR_HAZARDS if x.name == name)
        seam, length = S.error_seam(cls, s)
        assert len(d.data) == length and d.data[seam - s:seam - s + len(h.haz)] == h.haz, d.name
        assert seam % S.CHUNK == 0 and (cls == "chunk") == (seam % S.UNIT != 0)
        assert (cls == "block") == (seam % (S.BLOCK_UNITS * S.UNIT) == 0)
        seen.add(d.info)
    assert seen == {(h.name, s, cls) for h in S.ERROR_HAZARDS for s in S.splits(h) for cls in S.ERROR_CLASSES}
    names = {h.name for h in S.ERROR_HAZARDS}
    assert names == {"bad_letter", "nonhex_0", "nonhex_1", "nonhex_2", "nonhex_3", "cut_1", "cut_2", "cut_3",
                     "high_then_plain", "high_then_close", "high_then_simple"}


def test_compaction_documents_cover_all_256_cases():
    cases = set()
    for d in S.compaction_docs():
        cases |= S.compaction_cases(d.data)
    assert cases >= {(p, o, pos) for p in range(16) for o in range(8) for pos in (0, 1)}
    d = S.unit_count_doc()
    counts = set(S.unit_emit_counts(d.data).tolist())
    assert {0, 1, 4095, 4096} <= counts, counts
    opens = np.bincount([o // S.UNIT for o, _ in S.string_tokens(d.data)])
    assert opens.max() == S.DENSEST_STRINGS + 1 == 1366  # "", from byte 0 on: an opening quote is the unit's last byte too


def test_patch_documents_are_what_they_claim():
    """unit 1 of every patch document lies inside one string; `simple` units hold only simple escapes, `mixed` ones at
    least one \\u as well; the first / last emitted byte of the unit is an escaped one where the name says so"""
    letters = set()
    firsts = lasts = 0
    for d in S.patch_docs():
        assert any(o < S.UNIT and c >= 2 * S.UNIT for o, c in S.string_tokens(d.data)), d.name
        assert (b"\\u" in d.data[S.UNIT - 1:2 * S.UNIT]) == (d.info == "mixed"), d.name
        em = S.emit_mask(d.data)
        e = np.nonzero(em[S.UNIT:2 * S.UNIT])[0]
        for i in range(S.UNIT, 2 * S.UNIT):  # escaped letters: emitted bytes behind a backslash that is not emitted
            if d.data[i - 1] == 0x5C and not em[i - 1] and em[i] and d.data[i] != 0x75:
                letters.add(d.data[i])
        if "first" in d.name:
            firsts += 1
            assert d.data[S.UNIT + e[0] - 1] == 0x5C, d.name  # the first emitted byte follows a backslash
        if "last" in d.name:
            lasts += 1
            # the unit's last byte is emitted and belongs to an escape: its backslash lies at most four bytes in front
            starter = int(np.nonzero(~em[:2 * S.UNIT])[0][-1])  # the last byte of the unit that emits nothing
            assert e[-1] == S.UNIT - 1 and d.data[starter] == 0x5C and 1 <= 2 * S.UNIT - 1 - starter <= 4, d.name
    assert letters == set(S.SIMPLE_LETTERS) and firsts >= 16 and lasts >= 8


def test_selective_documents_cover_every_place():
    pats = {d.info for d in S.sel_chunk_docs()}
    assert pats == {(n, c, p) for n in ("inside", "across") for c in (5, 64, 127) for p in range(16)}
    for d in S.sel_chunk_docs():
        name, c, pat = d.info
        base = c * S.CHUNK
        toks = [(o, cl) for o, cl in S.string_tokens(d.data)][1:]
        assert len(toks) == 4
        assert [int(b"\\" in d.data[o:cl]) for o, cl in toks] == [(pat >> j) & 1 for j in range(4)]
        if name == "inside":
            assert all(base <= o and cl < base + S.CHUNK for o, cl in toks)
        else:
            assert toks[0][0] < base <= toks[0][1] and toks[3][0] < base + S.CHUNK <= toks[3][1]
            assert b"\\" not in d.data[base:base + S.CHUNK] or pat & 6  # the outer strings' starters lie outside the chunk
            assert b"\\" not in d.data[base:toks[0][1]] and b"\\" not in d.data[toks[3][0]:base + S.CHUNK]
    seen, dists = set(), set()
    for n in S.SEL_UNITS:
        for place in S.SEL_PLACES:
            if not S.sel_place_applies(n, place):
                assert n < S.SEL_STEP_UNITS and place.endswith("64")
                continue
            at = S.sel_starter_at(n, place)
            o, cl = S._OPEN_AT, S._OPEN_AT + n * S.UNIT
            assert cl // S.UNIT - o // S.UNIT == n
            if at is not None:
                assert o < at < cl - 1
                dists |= {("open", at // S.UNIT - o // S.UNIT), ("close", cl // S.UNIT - at // S.UNIT)}
                if place == "from_open_64":
                    assert at // S.UNIT - o // S.UNIT == 64
                if place == "from_close_64":
                    assert cl // S.UNIT - at // S.UNIT == 64
            seen.add((n, place))
    assert seen == {(n, p) for n in S.SEL_UNITS for p in S.SEL_PLACES if S.sel_place_applies(n, p)}
    assert dists >= {(side, k) for side in ("open", "close") for k in (0, 63, 64, 65)}, sorted(dists)
    assert S.SEL_UNITS == (1, 2, 3, 63, 64, 65, 66, 128, 129)
    # the documents themselves (the short ones: the long ones are built by the tests that parse them)
    for d in S.sel_long_docs(max_units=3):
        n, place, dist = d.info
        toks = S.string_tokens(d.data)
        o, cl = max(toks, key=lambda t: t[1] - t[0])
        assert (o, cl) == (S._OPEN_AT, S._OPEN_AT + n * S.UNIT)
        assert d.data[o + 1:cl].count(b"\\") == (0 if place == "absent" else 1)
        assert sum(1 for a, b in toks if a // S.UNIT == o // S.UNIT) >= 4 and sum(1 for a, b in toks if a // S.UNIT == cl // S.UNIT) >= 3
    assert [d.data.count(b"\\") for d in S.sel_message_docs()] == [0, 1, 1, 1]
    for d in S.sel_quote_docs():
        kind, starter = d.info
        o, cl = S.string_tokens(d.data)[1]
        assert (cl == 2 * S.UNIT) if kind == "close0" else (o == 2 * S.UNIT - 1)
        assert (b"\\" in d.data[o:cl]) == starter


# ---- verdicts of the oracle ------------------------------------------------------------------------------------------------
def _plain_docs(long_units=None):
    for nd in (False, True):
        yield from S.rotation_docs(nd)
        for lead in (1, 63):
            yield S.lead_doc(lead, nd)
    yield from S.compaction_docs()
    yield S.unit_count_doc()
    yield from S.patch_docs()
    yield from S.sel_chunk_docs()
    yield from S.sel_long_docs(long_units)
    yield from S.sel_message_docs()
    yield from S.sel_quote_docs()


def test_model_agrees_with_the_oracle_on_every_plain_document():
    """every plain document is accepted, and expected_strings is the oracle's Strings.B in both copy modes (which also
    settles the model's emit mask: its popcount per string is the length of what json.loads gives)"""
    n = 0
    for d in list(_plain_docs()) + [S.big_doc()]:
        assert d.plain
        for copy in (True, False):
            ref = O.parse(d.data, ndjson=d.nd, copy_strings=copy)
            assert ref.rc == 0, (d.name, copy)
            want = S.expected_strings(d.data, copy)
            assert ref.strings.tobytes() == want, (d.name, copy)
            assert int(S.emit_mask(d.data, copy).sum()) == len(want), (d.name, copy)
        n += 1
    assert n > 2 * len(S.COMBOS) + 200
    assert len(S.big_doc().data) > 4 << 20


def test_error_documents_are_rejected():
    for d in S.error_docs():
        for copy in (True, False):
            assert O.parse(d.data, copy_strings=copy).rc != 0, (d.name, copy)


def test_golden_bodies_keep_their_verdict_on_the_seams():
    bodies = _bodies()
    verdict = {i: O.parse(S.bare_doc(b)).rc == 0 for i, b in enumerate(bodies)}
    assert True in verdict.values() and False in verdict.values()
    n = 0
    for d in S.quirk_docs(bodies):
        i, s, cls = d.info
        for copy in (True, False):
            assert (O.parse(d.data, copy_strings=copy).rc == 0) == verdict[i], (d.name, bodies[i], copy)
        n += 1
    assert n == 3 * sum(len(b) - b.index(b"\\") + 2 for b in bodies if b"\\" in b)


# ---- the host replay ---------------------------------------------------------------------------------------------------------
def test_host_replay_error_documents(L):
    for d in S.error_docs():
        check(L, d.data, False, d.name)
    for d in S.quirk_docs(_bodies()):
        check(L, d.data, False, d.name)


@pytest.mark.parametrize("nd", [False, True])
def test_host_replay_rotation_documents(L, nd):
    for d in S.rotation_docs(nd):
        check(L, d.data, nd, d.name)
    for lead in (1, 63):  # (the replay has no lead: the same bytes at lead 0 put the hazards elsewhere, which costs nothing)
        d = S.lead_doc(lead, nd)
        check(L, d.data, nd, d.name)


def test_host_replay_compaction_and_patch_documents(L):
    for d in list(S.compaction_docs()) + [S.unit_count_doc()] + list(S.patch_docs()):
        check(L, d.data, False, d.name)


def test_host_replay_selective_documents(L):
    for d in list(S.sel_chunk_docs()) + list(S.sel_message_docs()) + list(S.sel_quote_docs()):
        check(L, d.data, False, d.name)
    for d in S.sel_long_docs():
        check(L, d.data, False, d.name)
