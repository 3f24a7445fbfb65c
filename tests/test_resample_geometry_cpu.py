"""The resampler's launch shape on the host (no GPU): `jat_k_resample_geometry` — which calls the functions `jat_resample`
launches by — against a restatement of DESIGN.md section 11's rules written here; the figures tests/resample_cases.py quotes
for each case; the completeness of that table (every branch of csrc/resample.hip's launch code is reached by a named case, so
a retune that moves a case off its branch fails here); and the refusals of `jat_resampler_create`."""
import ctypes as C
import math
import os

import pytest

import jatsr_amd._lib as L
import resample_cases as RC

FRAMES, TAP_TILE, MAX_THREADS, MAX_WINDOW = 8, 8, 256, 12288      # DESIGN.md section 11, "Launch shape"
FIELDS = ("K", "ph", "pn", "slices", "lanes", "groups_max", "groups", "grid_x", "block", "lds_bytes")


@pytest.fixture(scope="session")
def built_lib():
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return L.lib()


def library_shape(lib, case, n_in):
    """-> (rc, {field: value}) of jat_k_resample_geometry"""
    v = [C.c_int32(-1) for _ in FIELDS]
    rc = lib.jat_k_resample_geometry(case[0], case[1], case[2], case[3], n_in, *(C.byref(x) for x in v))
    return rc, {f: x.value for f, x in zip(FIELDS, v)}


# ---- the restatement ------------------------------------------------------------------------------------------------------
def dims(case):
    orig, new, lpw, rolloff = case
    g = math.gcd(orig, new)
    o, n = orig // g, new // g
    width = int(math.ceil(lpw * o / (min(o, n) * rolloff)))
    return o, n, width, 2 * width + o


def window(groups, o, K):
    return (groups * FRAMES - 1) * o + K


def block_shape(case):
    """-> dict, or None where even one frame group's window does not fit"""
    o, n, _, K = dims(case)
    ph = 4 if n >= 32 else 1
    cap = MAX_THREADS * ph
    slices = -(-n // cap)
    pn = -(-n // slices)                 # the phases spread evenly over the fewest slices
    slices = -(-n // pn)
    lanes = -(-pn // ph)
    by_threads = MAX_THREADS // lanes
    groups = by_threads
    while groups > 1 and window(groups, o, K) > MAX_WINDOW:
        groups -= 1
    if window(groups, o, K) > MAX_WINDOW:
        return None
    return dict(K=K, ph=ph, pn=pn, slices=slices, lanes=lanes, groups_max=groups, by_threads=by_threads)


def launch_shape(case, n_in):
    """-> dict of the launch for rows of n_in samples, with `want` (the frame groups asked for before the wave-fill rule)"""
    o, n, _, K = dims(case)
    s = block_shape(case)
    n_out = -(-n * n_in // o)
    n_frames = -(-n_out // n)
    want = min(max(n_frames // (FRAMES * 768), 1), s["groups_max"])
    groups = want
    for c in range(want, s["groups_max"] + 1):      # the first count that leaves at most 15 % of the last wave idle
        t = s["lanes"] * c
        if t * 100 >= -(-t // 64) * 64 * 85:
            groups = c
            break
    fpb = groups * FRAMES
    return dict(s, groups=groups, grid_x=-(-n_frames // fpb), block=s["lanes"] * groups, lds_bytes=4 * window(groups, o, K),
                want=want, n_frames=n_frames)


def lengths(case):
    """input lengths that cover: nothing but the first block, several blocks, and the first want > 1"""
    o = dims(case)[0]
    return [1, 7 * o + 3, 100 * o + 1, 12287 * o, 12288 * o, 3 * 12288 * o + 5]


# ---- every case against the restatement -------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [c for c, _ in RC.CASES], ids=RC.IDS)
def test_library_shape_is_the_restatement(built_lib, case):
    for n_in in lengths(case):
        rc, got = library_shape(built_lib, case, n_in)
        ref = launch_shape(case, n_in)
        assert rc == 0 and got == {f: ref[f] for f in FIELDS}, (case, n_in, got, ref)
        assert 1 <= got["groups"] <= got["groups_max"] and got["block"] <= MAX_THREADS and got["lds_bytes"] <= 4 * MAX_WINDOW
    rc, got = library_shape(built_lib, case, 0)                       # L = 0 launches nothing
    assert rc == 0 and (got["groups"], got["grid_x"], got["block"], got["lds_bytes"]) == (0, 0, 0, 0)
    assert got["groups_max"] == block_shape(case)["groups_max"]
    assert built_lib.jat_k_resample_geometry(*case, 100, *([None] * 10)) == 0     # every output is optional


# the figures tests/resample_cases.py and DESIGN.md quote: (orig, new, lpw) -> fields of the block shape (and o, n)
PINNED = {
    (47952, 44100, 6): dict(o=1332, n=1225, K=1346, ph=4, pn=613, slices=2, lanes=154, groups_max=1),
    (44100, 47952, 6): dict(o=1225, n=1332, ph=4, pn=666, slices=2, lanes=167),
    (11025, 96000, 6): dict(n=1280, pn=640, slices=2, lanes=160),
    (1000, 2049000, 6): dict(o=1, n=2049, pn=683, slices=3, lanes=171),
    (4000, 132300, 6): dict(n=1323, pn=662, slices=2, lanes=166),
    (1000, 31000, 6): dict(n=31, ph=1, lanes=31, groups_max=8),
    (1000, 32000, 6): dict(n=32, ph=4, lanes=8),
    (1000, 33000, 6): dict(n=33, ph=4, lanes=9),
    (8000, 48000, 6): dict(n=6, ph=1, lanes=6),
    (48000, 32000, 6): dict(o=3, n=2, ph=1, lanes=2, groups_max=128),
    (22050, 44100, 1): dict(o=1, n=2, K=5),
    (48000, 8000, 6): dict(n=1, K=80),
    (5000, 220500, 6): dict(n=441, K=24),
    (48000, 100, 6): dict(o=480, n=1, K=6300, groups_max=1),
    (96000, 11025, 6): dict(o=1280, n=147, K=1386, groups_max=1),
    (16000, 44100, 6): dict(o=160, n=441, K=174),
    (44100, 16000, 6): dict(o=441, n=160, K=475, lanes=40, groups_max=3),
    (48000, 16000, 6): dict(o=3, n=1, K=41),
    (44100, 48000, 6): dict(o=147, n=160, K=161, groups_max=6),
}
PINNED_WINDOW = {(47952, 44100, 6): 10670, (48000, 100, 6): 9660, (96000, 11025, 6): 10346}


def test_the_quoted_figures(built_lib):
    assert sorted(PINNED) == sorted(c[:3] for c, _ in RC.CASES)
    for case, _ in RC.CASES:
        o, n, _, K = dims(case)
        rc, got = library_shape(built_lib, case, 1000)
        assert rc == 0
        got.update(o=o, n=n)
        for f, v in PINNED[case[:3]].items():
            assert got[f] == v, (case, f, got[f], v)
        if case[:3] in PINNED_WINDOW:
            assert window(got["groups_max"], o, K) == PINNED_WINDOW[case[:3]]
    # the ragged cuts: 613 + 612, 662 + 661, three times 683
    assert 1225 - 613 == 612 and 1323 - 662 == 661 and 3 * 683 == 2049


# ---- the table reaches every branch -------------------------------------------------------------------------------------------
def test_the_case_table_is_complete(built_lib):
    shapes = []
    for case, why in RC.CASES:
        assert why.strip()
        o, n, _, K = dims(case)
        rc, s = library_shape(built_lib, case, 1000)
        assert rc == 0
        shapes.append(dict(s, o=o, n=n, case=case, by_threads=MAX_THREADS // s["lanes"]))

    def some(pred):
        return [s["case"] for s in shapes if pred(s)]

    assert some(lambda s: s["slices"] == 2 and s["n"] == 2 * s["pn"])                       # an even cut
    assert some(lambda s: s["slices"] >= 2 and s["n"] % s["pn"] != 0)                       # a shorter last slice
    assert some(lambda s: s["slices"] == 3)
    assert some(lambda s: s["slices"] >= 2 and s["ph"] * s["lanes"] > s["pn"])              # q < pn bites
    assert some(lambda s: s["slices"] >= 2 and s["n"] % s["pn"] != 0 and s["ph"] * s["lanes"] > s["pn"])   # both guards
    assert some(lambda s: s["ph"] == 1 and s["lanes"] > 3)
    for n in (31, 32, 33):
        assert some(lambda s: s["n"] == n), n
    assert some(lambda s: s["n"] == 31 and s["ph"] == 1) and some(lambda s: s["n"] == 32 and s["ph"] == 4)
    assert some(lambda s: s["K"] < TAP_TILE)
    assert some(lambda s: s["K"] % TAP_TILE == 0 and s["n"] == 1) and some(lambda s: s["K"] % TAP_TILE == 0 and s["n"] > 32)
    assert some(lambda s: s["groups_max"] == 1 and window(1, s["o"], s["K"]) > MAX_WINDOW // 2)
    assert some(lambda s: 1 < s["groups_max"] < s["by_threads"])                            # cut down by the window
    # launch groups > 1 chosen through want > 1: a length whose want = m > 1 gives more groups than the wave-fill rule alone
    # (want = 1) does.  case -> (groups at want 1, the first such m, groups there)
    through_want = {}
    for s in shapes:
        first = library_shape(built_lib, s["case"], 6144 * s["o"])[1]["groups"]
        for m in range(2, s["groups_max"] + 1):
            ref, got = launch_shape(s["case"], m * 6144 * s["o"]), library_shape(built_lib, s["case"], m * 6144 * s["o"])[1]
            assert ref["want"] == m and got["groups"] == ref["groups"] >= m
            if got["groups"] != first:
                through_want[s["case"][:2]] = (first, m, got["groups"])
                break
    assert through_want[(16000, 44100)] == (1, 2, 2)                 # at 12288 frames: 1.97 M input samples
    assert through_want[(48000, 16000)] == (55, 56, 56)              # n = 1: 55 groups fill a wave to 85 %; 1.03 M input samples
    assert through_want[(44100, 48000)] == (3, 4, 6)                 # 3.6 M input samples
    assert through_want[(1000, 31000)] == (2, 3, 4)                  # the cheapest: 18432 input samples
    # the rest never launch with another count: one group at most, or the wave-fill rule lands on the largest count
    assert sorted(set(s["case"][:2] for s in shapes) - set(through_want)) == sorted(
        [(47952, 44100), (44100, 47952), (11025, 96000), (1000, 2049000), (4000, 132300), (48000, 100), (96000, 11025),
         (44100, 16000)])


# ---- refusals -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,win", RC.REFUSED, ids=[f"{c[0]}-{c[1]}" for c, _ in RC.REFUSED])
def test_a_window_that_fits_no_block_is_refused_at_create(built_lib, case, win):
    o, n, _, K = dims(case)
    assert 7 * o + K == win > MAX_WINDOW and n * K <= 1 << 26 and block_shape(case) is None
    handle = C.c_void_p(0xDEAD)
    assert built_lib.jat_resampler_create(*case, None, C.byref(handle)) == L.JAT_E_INVALID and not handle.value
    text = built_lib.jat_last_error().decode()
    assert "window" in text and str(K) in text and str(o) in text and str(MAX_WINDOW) in text, text
    rc, got = library_shape(built_lib, case, 1000)
    assert rc == L.JAT_E_INVALID and set(got.values()) == {-1}                              # nothing written
    assert "window" in built_lib.jat_last_error().decode()
    d = [C.c_int32() for _ in range(4)]
    assert built_lib.jat_resample_table(*case, None, *(C.byref(x) for x in d)) == 0         # the table alone is fine


def test_the_other_refusals_are_those_of_create(built_lib):
    # 8001 and 44100 share 63, not 3: o = 127, and the conversion is served
    assert dims((8001, 44100, 6, 0.99))[:2] == (127, 700) and library_shape(built_lib, (8001, 44100, 6, 0.99), 1000)[0] == 0
    for case in ((0, 44100, 6, 0.99), (16000, -1, 6, 0.99), (16000, 44100, 0, 0.99), (16000, 44100, 6, 1.5),
                 (44101, 44100, 6, 0.99)):                                                  # the last: a table of 2e9 entries
        handle = C.c_void_p()
        assert built_lib.jat_resampler_create(*case, None, C.byref(handle)) == L.JAT_E_INVALID and not handle.value
        assert library_shape(built_lib, case, 1000)[0] == L.JAT_E_INVALID, case
    ok = (16000, 48000, 6, 0.99)                                                            # the lengths of jat_resample_out_length
    assert library_shape(built_lib, ok, -1)[0] == L.JAT_E_INVALID
    assert library_shape(built_lib, ok, 715827883)[0] == L.JAT_E_INVALID
    # the longest accepted row: L_out = 2^31 - 2, so L_out + n - 1 leaves 32 bits; n_frames = ceil(L_out / n) must not wrap
    rc, got = library_shape(built_lib, ok, 715827882)
    ref = launch_shape(ok, 715827882)
    assert rc == 0 and ref["n_frames"] == 715827882 and ref["want"] == ref["groups"] == ref["groups_max"] == 85
    assert got == {f: ref[f] for f in FIELDS} and got["grid_x"] == -(-715827882 // (8 * 85)) == 1052689
    rc, got = library_shape(built_lib, (44100, 44100, 6, 0.99), 1000)                       # a copy: no kernel
    assert rc == 0 and {f: v for f, v in got.items() if f != "K"} == dict.fromkeys(FIELDS[1:], 0)
