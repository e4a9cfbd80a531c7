"""CPU checks of tests/s1_geometry.py: the mirror of the stage-1 tile plan (csrc/stage1.hip s1_plan) covers every unit
exactly once on every branch, and the seam documents put every hazard where they say -- checked with the oracle.
Without these the GPU seam tests (tests/test_gpu_seams.py) could pass without ever touching a seam."""
import random

import numpy as np
import pytest

import oracle_lib as O
import s1_geometry as G

LEADS = (0, 1, 63)
CUS = (G.MI355X_CUS, 304, 80)


def _workspace_tiles(length):
    # csrc/stage1.hip stage1_workspace_bytes(len + 64) (api.hip): descriptors of one set
    return (length + 64 + 128) // (256 * 2 * 64) + 2 + 2048


def _lengths(variant, cus):
    out = []
    for units in G.branch_units(variant, cus).values():
        for lead in LEADS:
            out.append((units * G.UNIT - lead, lead))        # the last unit full
            out.append(((units - 1) * G.UNIT + 1 - lead, lead))  # one byte in the last unit
    return out


@pytest.mark.parametrize("cus", CUS)
@pytest.mark.parametrize("variant", range(len(G.S1_VARIANTS)))
def test_plan_covers_every_unit_once_in_order(variant, cus):
    rnd = random.Random(variant * 1000 + cus)
    cases = _lengths(variant, cus) + [(rnd.randrange(1, 70 << 20), rnd.choice(LEADS)) for _ in range(40)]
    branches = set()
    for length, lead in cases:
        if length < 1:
            continue
        p = G.plan(length, lead, variant, cus)
        branches.add(p.branch)
        tu = G.tile_units(p)
        assert [u for t in tu for u in t] == list(range(p.nu)), (length, lead, p)
        assert all(tu), ("a tile without a unit", length, lead, p)
        assert 1 <= p.su <= p.per_tile and p.tiles <= _workspace_tiles(length), p
        assert p.one_round == (p.tiles <= p.slots)
    assert branches == {"small", "fold_big_su", "rounds", "fold_few_units", "tail"}, branches


@pytest.mark.parametrize("variant", range(len(G.S1_VARIANTS)))
def test_branch_units_take_their_branch(variant):
    P, S = G.per_tile(variant), G.slots(variant, G.MI355X_CUS)
    for lead in LEADS:
        def pl(name):
            return G.plan(G.branch_units(variant)[name] * G.UNIT - lead, lead, variant)
        assert pl("su_per_tile_minus_1").su == P - 1 and pl("su_per_tile_minus_1").tiles == S
        assert pl("su_fold").branch == "fold_big_su"
        assert pl("one_round").tiles == S and pl("one_round").one_round
        assert pl("round_plus_1").tiles == S + 1 and not pl("round_plus_1").one_round
        assert pl("round_plus_slots_minus_1").branch == "fold_few_units"
        assert pl("round_plus_slots").branch == "tail" and pl("round_plus_slots").su == 1
        assert pl("round_plus_2_slots_plus_1").su == 3
        assert pl("two_rounds").tiles == 2 * S and pl("two_rounds").branch == "rounds"


def test_seam_document_has_every_class_for_every_variant():
    for cus in CUS:
        length = G.seam_doc_length(cus)
        for v in range(len(G.S1_VARIANTS)):
            for lead in range(64):
                p, sm = G.seams(length, lead, v, cus)
                assert p.branch == "tail" and 2 <= p.su < p.per_tile
                assert all(sm[c] for c in G.SEAM_CLASSES), (cus, v, lead, {c: len(sm[c]) for c in sm})
    assert length < 70 << 20


def test_seam_offsets_on_mi355x():
    """the offsets the suite never reached before (256 CUs, lead 0): the full/small seam and the last tile"""
    length = G.seam_doc_length()
    assert G.all_tail_units() == 8705
    want = {0: (33554432, 35651584), 1: (33554432, 35643392), 2: (25165824, 35618816), 5: (33554432, 35643392)}
    for v, (fs, last) in want.items():
        _, sm = G.seams(length, 0, v)
        assert sm["full_small"] == [fs] and sm["last_tile"] == [last], (v, sm["full_small"], sm["last_tile"])


def _combos_at(offset, lead0, lead, length):
    """(hazard, shift) that the rotation documents built for lead0 put around the seam at `offset` seen at `lead`"""
    n = G.units_of(length, lead0)
    cs = G.combos()
    u = (offset + lead) // G.UNIT
    assert u * G.UNIT - lead == offset and 1 <= u < n
    out = set()
    for k in range(len(cs)):
        h, s = cs[(u + k) % len(cs)]
        d = s + (lead - lead0)  # the seam is at u * 4096 - lead, the anchor at u * 4096 - lead0 + s
        if -2 <= d <= 2:
            out.add((h, d))
    return out


def test_rotation_puts_every_hazard_and_shift_on_every_seam_class():
    length = G.seam_doc_length()
    want = {(h, s) for h in G.HAZARDS for s in range(-2, 3)}
    for lead0, leads in ((0, (0, 1)), (63, (63,))):
        for nd in (False, True):  # nothing is left out: the rotation targets are 4 KiB apart
            for k in (0, len(G.combos()) - 1):
                tg = G.rotation_targets(length, lead0, k)
                assert len(G.place(length, tg, nd)) == len(tg)
        for lead in leads:
            for v in range(len(G.S1_VARIANTS)):
                _, sm = G.seams(length, lead, v)
                for cls in G.SEAM_CLASSES:
                    if cls == "end":
                        continue
                    for off in sm[cls][:3] + sm[cls][-3:]:
                        assert _combos_at(off, lead0, lead, length) == want, (lead, v, cls, off)
    # the message end: every hazard ends 0 .. 5 bytes in front of the closing bracket in some document
    ends = set()
    for k in range(len(G.combos())):
        t = G.message_end_targets(length, k)
        pl = G.place(length, G.rotation_targets(length, 0, k) + [t])
        assert pl[-1].target == t
        text, anchor, _ = G.HAZARDS[t.hazard](False)
        ends.add((t.hazard, length - 1 - (pl[-1].start + len(text))))
    assert ends == {(h, d) for h in G.HAZARDS for d in range(6)}


def _check_anchors(data, placed, nd):
    ok, pos = O.stage1(data, nd)
    assert ok
    s = set(int(p) for p in pos)
    for pl in placed:
        assert (pl.anchor_at in s) == pl.structural, (pl, nd)
    return pos


@pytest.mark.parametrize("nd", [False, True])
def test_every_hazard_at_every_shift_is_where_it_claims(nd):
    """small documents, one hazard on one 4 KiB seam: the anchor byte is (or is not) a structural as the hazard says,
    and the document is valid"""
    for h in G.HAZARDS:
        for s in G.SHIFTS:
            a, placed = G.byte_doc(3 * G.UNIT + 100, [G.Target(G.UNIT, h, s), G.Target(2 * G.UNIT, h, -s)], nd)
            assert len(placed) == 2 and len(a) == 3 * G.UNIT + 100
            assert placed[0].anchor_at == G.UNIT + s
            _check_anchors(a, placed, nd)
            assert O.parse(a, ndjson=nd).rc == 0, (h, s, nd)


@pytest.mark.parametrize("nd", [False, True])
def test_error_hazards_are_errors(nd):
    for h in G.ERROR_HAZARDS:
        for s in (-1, 0, 1):
            a, placed = G.byte_doc(3 * G.UNIT, [G.Target(G.UNIT, h, s)], nd)
            assert len(placed) == 1
            assert not O.stage1(a, nd)[0] and O.parse(a, ndjson=nd).rc != 0


@pytest.mark.parametrize("lead0,k,nd", [(0, 0, False), (63, 7, True), (0, 41, True)])
def test_full_size_seam_documents(lead0, k, nd):
    a, placed = G.byte_seam_doc(k, lead0, nd)
    assert len(a) == G.seam_doc_length() and len(placed) == G.units_of(len(a), lead0)
    _check_anchors(a, placed, nd)
    assert O.parse(a, ndjson=nd).rc == 0


def test_sparse_documents_leave_whole_units_blank():
    """blank runs longer than a unit in front of a seam of every class (of some variant)"""
    length = G.seam_doc_length()
    for lead in (0, 63):
        a, placed = G.sparse_doc(length, lead, range(len(G.S1_VARIANTS)))
        pos = _check_anchors(a, placed, False).astype(np.int64)
        assert O.parse(a).rc == 0
        blank = {}
        for v in range(len(G.S1_VARIANTS)):
            _, sm = G.seams(length, lead, v)
            for cls in ("full_small", "last_tile", "small", "full", "unit_small"):
                i = np.searchsorted(pos, np.array(sm[cls], dtype=np.int64) - 100)  # the first structural of a hazard
                blank[cls] = blank.get(cls, False) or bool(np.any(pos[i] - pos[i - 1] > G.UNIT))  # on the seam
        assert all(blank.values()), (lead, blank)


@pytest.mark.parametrize("nd", [False, True])
@pytest.mark.parametrize("kind", sorted(G.TOKEN_KINDS))
def test_token_documents_put_the_kind_on_the_stage2_seams(kind, nd):
    if kind in G.ND_ONLY and not nd:
        return
    for d in G.TOKEN_OFFSETS:
        data, idx, offs = G.token_doc(kind, d, O.stage1, nd=nd)
        ok, pos = O.stage1(data, nd)
        assert ok
        assert [int(pos[i]) for i in idx] == offs, (kind, d)
        assert idx == [G.S2_TILE * t + d for t in (1, 2, 3)]
        assert (len(pos) - 1) // G.S2_TILE == 3
        assert O.parse(data, ndjson=nd).rc == 0, (kind, d, nd)


def test_nesting_documents():
    for depth in (4095, 4096, 4097):
        data = G.nesting_doc(depth)
        ok, pos = O.stage1(data)
        assert ok and len(pos) == 2 * depth and data[int(pos[4095])] == ord("[" if depth > 4095 else "]")
        assert O.parse(data).rc == 0
