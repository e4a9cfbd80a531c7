"""CPU: the documents of tests/ms_geometry.py lie where they claim to lie and say what the oracle says.

For every document the oracle parses it, the oracle's tape has the builder's tags on the builder's words (and the builder's
Strings.B offsets and lengths in its string entries), and the oracle's MarshalJSON is the builder's text byte for byte -- so the
two references of tests/test_gpu_marshal_seams.py agree before the device is asked.  The coverage tests compute, from the
documents themselves, which cut of k_ms_tile each of them reaches, and compare that with what the families promise; the
constants the placements rest on are pinned to the literals in csrc/marshal.hip and csrc/sj_tapewalk.h."""
import functools
import os

import numpy as np
import pytest

import ms_geometry as M
import oracle_lib as O
import tape_reader as TR

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "simdjson-go_amd", "csrc")


@functools.lru_cache(maxsize=None)
def docs(f):
    return list(M.family(f))


@functools.lru_cache(maxsize=None)
def ref(f, i):
    d = docs(f)[i]
    r = O.parse(d.data, ndjson=d.nd, copy_strings=True)
    assert r.rc == 0, d.name
    return r


def test_escape_and_its_inverse():
    s = bytes(range(0x80))
    assert M.escape(b'a"\\/\b\f\n\r\t\x00\x1f\x7f') == b'a\\"\\\\/\\b\\f\\n\\r\\t\\u0000\\u001f\x7f'
    assert M.unescape(M.escape(s)) == s


@pytest.mark.parametrize("f", sorted(M.FAMILIES))
def test_documents_agree_with_the_oracle(f):
    assert docs(f)
    for i, d in enumerate(docs(f)):
        r = ref(f, i)
        tape = r.tape
        assert len(tape) == M.n_words(d), d.name
        tags = np.array([ord(M.TAG[k]) for k in d.kinds], dtype=np.uint64)
        assert np.array_equal(tape[d.words] >> np.uint64(56), tags), d.name
        width = np.array([2 if k in M.TWO_WORD else 1 for k in d.kinds], dtype=np.int64)
        assert np.array_equal(d.words[1:], (d.words + width)[:-1]) and d.words[-1] + 1 == len(tape), d.name  # (no other entries)
        is_str = d.soffs >= 0
        pay = tape[d.words[is_str]] & np.uint64(TR.MASK)
        assert np.array_equal(pay, d.soffs[is_str].astype(np.uint64) | np.uint64(TR.STRINGBUFBIT)), d.name
        assert np.array_equal(tape[d.words[is_str] + 1], np.array([d.info["slen"][j] for j in np.flatnonzero(is_str)], dtype=np.uint64))
        assert len(r.strings) == d.info["strings_len"], d.name
        rc, want = O.marshal_json(tape, r.strings, d.data[r.msg_off:r.msg_off + r.msg_len])
        assert rc == 0 and want == d.text == b"".join(d.pieces), d.name
        if "tile_text" in d.info:
            assert M.tile_text_bytes(d)[d.info["tile"]] == d.info["tile_text"], d.name
        assert M.tile_text_bytes(d).sum() == len(d.text)
        k = len(d.text) // 2  # the reporter of the GPU test names the entry that owns a byte
        t, w, kind, j = M.owner(d, k)
        st = M.text_starts(d)
        assert st[j] <= k < st[j] + len(d.pieces[j]) and w == d.words[j] and t == w // M.TILE, d.name


def test_no_copy_mode_reads_the_message():
    """WithCopyStrings(false): only escaped strings lie in Strings.B, the others at their message offset; the last string of the
    message ends two bytes in front of its end"""
    for i, d in enumerate(docs("f")):
        r = O.parse(d.data, ndjson=d.nd, copy_strings=False)
        assert r.rc == 0 and r.msg_off == 0
        last = max(j for j in d.info["_bytes"])
        for j, s in d.info["_bytes"].items():
            w = int(r.tape[d.words[j]]) & TR.MASK
            if any(c in b'"\\' or c < 0x20 for c in s):
                assert w & TR.STRINGBUFBIT, (d.name, j)
            else:
                assert w == d.srcoffs[j] + 1, (d.name, j)
        if "tail" in d.info:
            assert int(d.srcoffs[last]) + 1 + d.info["tail"] == len(d.data) - 2


# ---- the constants -------------------------------------------------------------------------------------------------------------------
def test_constants_are_the_kernels():
    ms = open(os.path.join(CSRC, "marshal.hip")).read()
    tw = open(os.path.join(CSRC, "sj_tapewalk.h")).read()
    assert M.TILE == M.THREADS * M.ITEMS and M.QCAP == M.TILE // 2
    assert "static constexpr int TW_THREADS = %d, TW_ITEMS = %d, TW_TILE = TW_THREADS * TW_ITEMS;" % (M.THREADS, M.ITEMS) in tw
    assert "static constexpr u32 MS_QCAP = TW_TILE / 2;" in ms
    assert "static constexpr u32 MS_LONG = %d;" % M.MS_LONG in ms
    assert "static constexpr u32 MS_WINDOW = %d;" % M.VARIANTS[0][0] in ms
    assert "if (base + TW_ITEMS + 2 <= p.n) {" in ms  # the vector load of a thread's words: base + 10 <= n
    assert "case 1: hipLaunchKernelGGL((k_ms_tile<MODE, 3, MS_WINDOW>)" in ms
    assert "case 3: hipLaunchKernelGGL((k_ms_tile<MODE, 4, MS_WINDOW / 2>)" in ms and M.VARIANTS[3][0] == M.VARIANTS[0][0] // 2
    assert "case 5: hipLaunchKernelGGL((k_ms_tile<MODE, 4, %du>)" % M.VARIANTS[5][0] in ms
    assert "case 6: hipLaunchKernelGGL((k_ms_tile<MODE, 4, %du>)" % M.VARIANTS[6][0] in ms
    assert "case 7: hipLaunchKernelGGL((k_ms_tile<MODE, 4, %du, %du>)" % M.VARIANTS[7] in ms
    assert sorted(w for w, _ in M.VARIANTS.values()) == sorted(M.WINDOWS) and M.VARIANTS[7][1] == M.STAGE
    # the default launch
    assert ("if (p.tiles && (u64)(p.strings_end - p.strings) / p.tiles <= %du && p.msg_len / p.tiles <= %du)\n"
            "                hipLaunchKernelGGL((k_ms_tile<MODE, 4, %du, %du>), g, b, 0, st, p);\n"
            "            else\n"
            "                hipLaunchKernelGGL((k_ms_tile<MODE, 4, %du>), g, b, 0, st, p);"
            % ((M.STAGED_MAX_STRINGS_PER_TILE, M.STAGED_MAX_MSG_PER_TILE) + M.default_form(0, 0, 1) + M.default_form(1 << 20, 0, 1)[:1])) in ms
    # the anchor search: one word per thread of wave 0, REACH words in front of the tile
    assert "const bool a_have = tid < %d && !p.tile_last && tb >= 1 + (u64)tid;" % M.REACH in ms
    assert "(tb > %d ? -2ll : -1ll)" % M.REACH in ms
    # the look-back: LOOKBACK descriptors per step
    assert "const long long idx = j - lane;" in ms and "        j -= %d;" % M.LOOKBACK in ms
    # the stage
    assert "off - st_base + %d <= (u64)st_avail" % M.STAGE_HEAD in ms
    assert "st_base = (u64)(lo & ~15u);" in ms and "st_avail = (u32)(left < STAGE ? left & ~15ull : (u64)STAGE);" in ms
    # long strings: a wave, LONG_STEP bytes per step
    assert "for (u64 c0 = 0; c0 < len; c0 += %d) {" % M.LONG_STEP in ms and "q < len; q += %d)" % M.LONG_STEP in ms
    assert "const bool lng = w[k + 1] >= MS_LONG;" in ms
    # the key tiles
    assert "const u32 base = blockIdx.x * %du + (u32)tid * %du;" % (M.KEY_TILE, M.KEY_ITEMS) in ms
    assert "kv.tiles = (kv.n + %du) / %du;" % (M.KEY_TILE - 1, M.KEY_TILE) in ms


# ---- coverage ------------------------------------------------------------------------------------------------------------------------
def test_a_every_kind_on_every_edge():
    by = {d.name: d for d in docs("a")}
    for cls in ("tile", "thread"):
        for nd in (False, True):
            d = by["a %s edges%s" % (cls, " nd" if nd else "")]
            want = set(M.a_cases(nd))
            assert want - M.a_observed(d, cls) == set(), (d.name, sorted(want - M.a_observed(d, cls)))
            for kind, pos, follow, edge in d.info["lay"]:  # ... and each where the layout says
                hit = [i for i, w in enumerate(d.words) if w == edge - pos and d.kinds[i] == (kind if kind not in "Rr" else kind)]
                assert hit and (edge % M.TILE == 0) == (cls == "tile"), (d.name, kind, pos, edge)
    kinds = {k for k, _, _ in M.a_cases(True)}
    assert kinds == set(M.A_KINDS) | {"R", "r"} and {"str", "key", "int", "uint", "float", "true", "false", "null", "[", "{", "]", "}"} <= kinds
    ns = {M.n_words(d) for d in docs("a")}
    assert {n % M.TILE for n in ns if n > M.TILE} >= set(M.A_RESIDUES) and set(range(4, 10)) <= ns
    zero = [d for d in docs("a") if M.n_words(d) % M.TILE == 1]
    assert zero and all(M.tile_text_bytes(d)[-1] == 0 for d in zero)  # the last tile: the closing root only
    d = by["a nd four-word records"]
    i = list(d.words).index(M.TILE - 1)
    assert d.kinds[i] == "R" and d.kinds[i + 1] == "r" and d.words[i + 1] == M.TILE
    assert all(d.words[j] % 4 == 0 for j, k in enumerate(d.kinds) if k == "r")


def test_b_anchor_distances_and_tops():
    seen, tops = set(), set()
    for i, d in enumerate(docs("b")):
        tape = ref("b", i).tape
        if "run" in d.info:
            edge, anchor = d.info["edge"], d.info["anchor"]
            two = np.isin(tape >> np.uint64(56), np.array(M.TWO_WORD_TOPS, dtype=np.uint64))
            assert not two[anchor] and two[anchor + 1:edge + 2].all(), d.name  # the closest anchor in front of the edge
            assert edge - anchor == M.b_distance(d.info["run"], d.info["parity"])
            assert d.info["local"] == (edge - anchor <= M.REACH) and M.n_tiles(d) == 3
            raw_first = int(edge) not in set(d.words.tolist())  # parity 1: the edge splits an entry
            assert raw_first == bool(d.info["parity"])
            seen.add((d.info["run"], d.info["parity"], edge // M.TILE, d.info["local"]))
        else:
            tops |= M.b_observed_tops(d, tape)
    assert {s[:3] for s in seen} == {(r, p, t) for r in M.B_RUNS for p in (0, 1) for t in (1, 2)}
    # 31 entries: inside the reach; 32: the farthest word the search sees (parity 1) or one beyond it; 33: beyond
    assert {(r, p): l for r, p, _, l in seen} == {(31, 0): True, (31, 1): True, (32, 0): False, (32, 1): True, (33, 0): False, (33, 1): False}
    assert M.b_distance(32, 1) == M.REACH
    assert tops >= {(t, s) for t in M.ONE_WORD_TOPS for s in ("front", "first")}


def test_c_window_edges():
    seen = set()
    for d in docs("c"):
        tt = M.tile_text_bytes(d)
        if "window" in d.info:
            assert tt[1] == d.info["window"] + d.info["delta"] and tt[0] < 4096 and tt[2] < 64 + (M.C_TAIL if d.info["window"] == 21504 else 0) and M.n_tiles(d) == 3
            assert {k for k, w in zip(d.kinds, d.words) if w // M.TILE == 1} >= set(M.A_KINDS)
            seen.add((d.info["window"], d.info["delta"]))
        else:
            assert all(k not in ("str", "key") for k, w in zip(d.kinds, d.words) if w // M.TILE == 1)
    assert seen == {(w, dl) for w in M.WINDOWS for dl in (-1, 0, 1)}
    short = sorted(int(M.tile_text_bytes(d)[1]) for d in docs("c") if "window" not in d.info)
    assert short[0] > 16384 and short[1] > 21504  # over the windows of the default forms: literals and numbers straight to memory
    for d in docs("c"):  # the default launch takes the large window for the 21504 documents
        if d.info.get("window") == 21504:
            assert M.default_form(d.info["strings_len"], len(d.data), M.n_tiles(d)) == (21504, 0)


def test_d_every_offset_length_and_escape():
    by = {d.info["part"] + str(d.info.get("fits", "")): d for d in docs("d")}
    obs = M.d_observed(by["clean"], 0, M.MS_LONG)
    want = {(o, n, (), "str", True) for o in range(8) for n in M.D_LENGTHS} | {(o, n, (), "str", False) for o in range(8) for n in M.D_LENGTHS} \
        | {(o, n, (), "key", True) for o in range(8) for n in M.D_LENGTHS}
    assert want - obs == set()
    obs = {x[:3] for x in M.d_observed(by["one"], 0, M.MS_LONG)}
    assert {(o, n, (p,)) for o in range(8) for n in M.D_LENGTHS for p in range(n)} - obs == set()
    obs = {x[:3] for x in M.d_observed(by["three"], 0, M.MS_LONG)}
    assert {(o, n, (7, 8, 9)) for o in range(8) for n in M.D_LENGTHS if n >= 10} - obs == set()
    for d in (by["clean"], by["one"], by["three"], by["longTrue"]):
        assert M.tile_text_bytes(d).max() <= min(M.WINDOWS), d.name
    assert (M.tile_text_bytes(by["longFalse"])[:-1] > max(M.WINDOWS)).all()
    want = {(o, n, () if q is None else (q,)) for o in range(8) for n, q in M.d_long_cases()}
    assert {n for n, _ in M.d_long_cases()} == set(M.D_LONG_LENGTHS)
    for key in ("longTrue", "longFalse"):
        assert want - {x[:3] for x in M.d_observed(by[key], M.MS_LONG, 30000)} == set(), key
    d = by["other"]
    rel = M.tile_rel_offsets(d)
    obs = {(k, int(r) % 8) for k, r, p in zip(d.kinds, rel, d.pieces) if p}
    assert {(k, o) for k in ("true", "false", "null", "[", "{", "]", "}", "int", "uint", "float", "R") for o in range(8)} - obs == set()
    assert all(p.endswith(b",") for k, p in zip(d.kinds, d.pieces) if k in ("int", "uint", "float"))


def test_e_queue_splits():
    obs = {M.e_observed(d) for d in docs("e")}
    q = M.QCAP
    want = {(q, 0, 0, 0), (0, q, 0, 0), (0, 0, q, 0), (0, 0, 0, q)}
    want |= {(a, b, q - a - b, 0) for a, b in M.E_SPLITS} | {(0, 0, a, b) for a, b in M.E_SPLITS}
    want |= {(n, 0, q - n, 0) for n in M.E_SHORT_COUNTS} | {(0, n, 0, q - n) for n in M.E_LONG_COUNTS}
    assert want - obs == set(), sorted(want - obs)
    names = [d.name for d in docs("e")]
    assert sum("x empty" in n for n in names) == 1 and sum("x one" in n for n in names) == 1  # (two of the full short queues)
    for d in docs("e"):
        first = list(d.words).index(M.TILE)  # tile 1 starts on an entry and holds 1024 two-word entries
        assert list(d.words[first:first + q]) == list(range(M.TILE, 2 * M.TILE, 2)), d.name
        if "key_last" in d.info:
            assert M.e_observed(d) == (q, 0, 0, 0)
            assert d.kinds[first + q - 1] == ("key" if d.info["key_last"] else "str")  # ordinal 1023
            assert sum(k == "key" for k in d.kinds[first:first + q]) == q // 2
    assert {d.info["key_last"] for d in docs("e") if "key_last" in d.info} == {True, False}


def test_f_stage_and_buffer_ends():
    dist, lo16, tails, straddle = set(), set(), set(), 0
    for d in docs("f"):
        # the default launch takes the staged form (launch_ms_tile: Strings.B and message bytes per tile)
        assert M.default_form(d.info["strings_len"], len(d.data), M.n_tiles(d)) == (13312, M.STAGE), d.name
        for t, (base, avail, lo, strs) in M.stage_ranges(d).items():
            cut = avail < M.STAGE
            assert base % 16 == 0 and avail % 16 == 0 and base + avail <= d.info["strings_len"]
            for j, dd in strs:
                if dd in M.F_DISTANCES and d.info.get("dist") == dd and d.info["slen"][j] == 16:
                    assert cut == d.info["cut"], d.name
                    dist.add((dd, cut))
            if "lo" in d.info and t == 1:
                lo16.add(lo % 16 if d.info["lo"] < 16 else 16 * (lo // 16 - 160 // 16) + lo % 16)
            if "straddle" in d.info and t == 1:
                straddle = sum(dd > 0 for _, dd in strs), len(strs)
        if "tail" in d.info:
            last = max(d.info["slen"])
            assert d.soffs[last] + d.info["slen"][last] == d.info["strings_len"] and d.info["slen"][last] == d.info["tail"]
            tails.add(d.info["tail"])
    assert dist == {(dd, cut) for dd in M.F_DISTANCES for cut in (False, True)}
    assert lo16 == set(M.F_LO_MOD16)
    assert tails == set(range(1, 17))
    assert straddle[0] > straddle[1] // 2  # most short strings of the tile lie beyond the staged range


def test_g_tile_counts():
    seen = {}
    for d in docs("g"):
        seen.setdefault(d.info["form"], set()).add(M.n_tiles(d))
        assert M.n_tiles(d) == d.info["tiles"] and len(d.data) < (1 << 20) + 700000
        tt = M.tile_text_bytes(d)
        if d.info["form"] == "zero":
            assert tt[-1] == 0 and M.n_words(d) % M.TILE == 1
        if d.info["form"] == "over":
            assert list(np.flatnonzero(tt > max(M.WINDOWS))) == [t for t in range(d.info["tiles"]) if t % 7 == 3]
        if d.info["form"] == "plain":
            assert len(d.text) < 1 << 20 and 1.5 < len(d.text) / M.n_words(d) < 2.5
    assert seen == {"plain": set(M.G_TILES), "over": {65, 129}, "zero": {65, 129}}
    assert {1, 2, M.LOOKBACK - 1, M.LOOKBACK, M.LOOKBACK + 1, M.LOOKBACK + 2, 2 * M.LOOKBACK, 2 * M.LOOKBACK + 1, 2 * M.LOOKBACK + 2} == set(M.G_TILES)


def test_h_token_positions():
    seen = set()
    for d in docs("h"):
        ok, pos = O.stage1(d.data, ndjson=d.nd)
        assert ok
        strs = [i for i, k in enumerate(d.kinds) if k in ("key", "str")]
        for i in strs:  # the builder's token index of every string is the structural index's
            assert pos[d.toks[i]] == d.srcoffs[i] and d.data[pos[d.toks[i]]] == 0x22, (d.name, i)
            nxt = d.data[pos[d.toks[i] + 1]:pos[d.toks[i] + 1] + 1]
            assert (nxt == b":") == (d.kinds[i] == "key")
        if "lay" in d.info:
            at = {int(d.toks[i]): d.kinds[i] for i in strs}
            for kind, target in d.info["lay"]:
                assert at[target] == kind
                seen.add((kind, "tile" if target % M.KEY_TILE == M.KEY_TILE - 1 else "thread" if target % M.KEY_ITEMS == M.KEY_ITEMS - 1 else None))
        else:
            assert int(d.toks[strs[-1]]) == len(pos) - 2  # only the closing bracket behind the last string token
    assert seen == {("key", "tile"), ("key", "thread"), ("str", "tile"), ("str", "thread")}


def test_i_number_sweep():
    fl, it = docs("i")
    bits = M.i_float_bits()
    assert len(bits) == len(set(bits)) + (len(bits) - len(set(bits))) and len(bits) >= 6 * 2047 + M.I_RANDOM
    binades = {(b >> 52) & 0x7FF for b in bits}
    assert binades == set(range(2047))
    assert np.array_equal(ref("i", 0).tape[fl.words[2:-2] + 1], np.array(bits, dtype=np.uint64))  # (the source round-trips)
    vals = set(M.i_ints())
    assert {10 ** k for k in range(20)} <= vals and {-(10 ** k) for k in range(19)} <= vals and {10 ** k - 1 for k in range(1, 20)} <= vals
    assert {(1 << 63) - 1, -(1 << 63), 1 << 63, (1 << 64) - 1} <= vals
