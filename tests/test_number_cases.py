"""CPU: the number texts of tests/number_cases.py.  The arbiter is proved once (Fraction arithmetic against float(str): nearest,
ties to even, no C library involved); then every family goes through the host replay of csrc/sj_number.h + sj_bignum.h
(sj_selftest_parse_number) and of csrc/sj_ftoa.h (sj_selftest_format_float), and through the oracle, against the arbiter's
words and go_format.  The conditions on the generator that tests/test_gpu_numbers.py relies on are asserted here."""
import ctypes as C

import pytest

import __graft_entry__ as G
import number_cases as N
import oracle_lib as O

u64p = C.POINTER(C.c_uint64)
BIG_QUEUE_TRIPS = 3 * 4096 + 1  # k_bignum walks its queue 64 blocks x 64 lanes at a time: more than three full trips


@pytest.fixture(scope="module")
def L():
    lib = C.CDLL(G.build_selftest())
    lib.sj_selftest_parse_number.argtypes = [C.c_char_p, C.c_size_t, u64p, u64p, C.POINTER(C.c_int)]
    lib.sj_selftest_format_float.argtypes = [C.c_uint64, C.c_char_p]
    lib.sj_selftest_format_float.restype = C.c_uint
    return lib


def host_parse(L, text):
    """-> ((tag word, value word) or None, took the big-integer path)"""
    b = text.encode() + b","
    t, v, big = C.c_uint64(), C.c_uint64(), C.c_int()
    st = L.sj_selftest_parse_number(b, len(b), C.byref(t), C.byref(v), C.byref(big))
    return ((t.value, v.value) if st else None), big.value


def oracle_parse(OL, text):
    b = text.encode() + b","
    v = C.c_uint64()
    t = OL.sjo_parse_number(b, len(b), C.byref(v))
    return (t, v.value) if t else None


def show(w):
    return "reject" if w is None else "%016x %016x" % w


def want_words(exp):
    return None if exp == "reject" else N.words(exp)


@pytest.fixture(scope="module")
def host_results(L):
    """{family: [((tag, value) or None, big-integer path), ...]}"""
    return {name: [host_parse(L, t) for t, _ in cases] for name, cases in N.families().items()}


def test_the_arbiter_is_correctly_rounded():
    """float(str) against Fraction(str): every text of the families built around ties and edges -- all exact ties among
    them -- and a sample of the random fill"""
    n = 0
    for name, cases in N.families().items():
        step = 40 if name == "random_fill" else 1
        for t, e in cases[::step]:
            if "e" in t.lower() and len(t.lower().split("e")[1]) > 5:
                continue  # (a zero with a huge exponent: nothing to round)
            want = N.rounded_bits(t)
            got = N.f2bits(float(t))
            assert got == want, (name, t[:60], "%016x" % got, "%016x" % want)
            assert e == "reject" if want & ~N.SIGN == N.INF_BITS else e != "reject", (name, t[:60])
            n += 1
    assert n > 100000, n


@pytest.mark.parametrize("name", N.FAMILIES)
def test_parse_on_the_host_replay_and_the_oracle(L, host_results, name):
    OL = O.lib()
    for (t, e), (got, _) in zip(N.families()[name], host_results[name]):
        want = want_words(e)
        assert got == want, "host replay: %s %s got %s want %s" % (name, t[:60], show(got), show(want))
        ref = oracle_parse(OL, t)
        assert ref == want, "oracle: %s %s got %s want %s" % (name, t[:60], show(ref), show(want))


@pytest.mark.parametrize("name", N.FAMILIES)
def test_format_on_the_host_replay_and_the_oracle(L, name):
    buf = C.create_string_buffer(40)
    seen = set()
    for t, e in N.families()[name]:
        if e == "reject":
            continue
        bits = e[1] if e[0] == "d" else N.f2bits(float(e[1]))
        if bits in seen:
            continue
        seen.add(bits)
        want = N.go_format(N.bits2f(bits))
        k = L.sj_selftest_format_float(bits, buf)
        assert k < 0x80000000, (name, hex(bits))  # (bytes behind the text were written, or the length-only form disagrees)
        got = buf.raw[:k].decode()
        assert got == want, "host replay: %s %016x got %s want %s" % (name, bits, got, want)
        ref = O.format_float(bits)
        assert ref == want, "oracle: %s %016x got %s want %s" % (name, bits, ref, want)
        assert N.f2bits(float(got)) == bits, (name, hex(bits), got)
    assert seen


def test_conditions_on_the_generator(host_results):
    fam = N.families()
    assert all(len(v) > 0 for v in fam.values())
    assert sum(len(v) for v in fam.values()) >= 300000
    # the density document of test_gpu_numbers.py: every member takes the big-integer path, and there are enough of them
    big = [b for _, b in host_results["tiebreak"]]
    assert all(big) and len(big) >= BIG_QUEUE_TRIPS, (sum(big), len(big))
    digits = [len(t.split("e")[0].replace(".", "").lstrip("-")) for t, _ in fam["tiebreak"]]
    assert min(digits) <= 24 and max(digits) >= 760
    assert all(e != "reject" for _, e in fam["tiebreak"])
    # the refine step: recomputed here for every member
    assert len(fam["refine"]) >= 1000
    for t, _ in fam["refine"]:
        w, q = (int(x) for x in t.split("e"))
        assert (((w << (64 - w.bit_length())) * N._pow5_hi64(q)) >> 64) & 0x1FF == 0x1FF, t
    every = [e for v in fam.values() for _, e in v]
    subnormal = sum(1 for e in every if e != "reject" and e[0] == "d" and 0 < (e[1] & ~N.SIGN) < (1 << 52))
    assert subnormal >= 300, subnormal
    assert sum(1 for e in every if e == "reject") >= 20
    doubles = {e[1] for e in every if e != "reject" and e[0] == "d"}
    assert len(doubles) > 250000  # (what the float printing sees)
    assert {e[0] for e in every if e != "reject"} == {"l", "u", "d"}
    assert any(e != "reject" and e[0] == "d" and e[2] == 1 for e in every)  # (the overflowed-integer flag)
    # every reject has its accepted neighbour
    for bad, good in N.reject_pairs():
        assert N.expect(bad) == "reject" and N.expect(good) != "reject", (bad[:60], good[:60])
    assert N.families() is N.families() and N.families.__wrapped__(20261016) == fam  # deterministic
