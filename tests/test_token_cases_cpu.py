"""No GPU: the specification of the device tokenisers (tests/token_cases.py) held against the host parser -- which
tests/test_reader_cpu.py pins to the reference -- against exact arithmetic and against np.loadtxt, and the coverage the
alignment files of tests/test_gpu_tokeniser.py claim, counted from their text for every offset a line can begin at."""
import gzip
import io
from fractions import Fraction

import numpy as np
import pytest

import token_cases as tc
from test_depth_reader_cpu import table_rows


def host_rows(tmp_path, text):
    from wgsassign_amd import reader_cy
    p = str(tmp_path / "f.beagle.gz")
    with gzip.open(p, "wb", compresslevel=1) as fh:
        fh.write(text)
    return reader_cy.readBeagle(p)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def check_host(tmp_path, case):
    rows, _, names = host_rows(tmp_path, case.text)
    assert rows.shape == case.want.shape
    bad = np.argwhere(bits(rows) != bits(case.want))
    assert bad.size == 0, (bad[:5], [(rows[r, c], case.want[r, c]) for r, c in bad[:5]])
    assert names == case.names


@pytest.mark.parametrize("name", sorted(tc.BEAGLE_CASES))
def test_the_host_parser_has_atof32s_bits_on_every_case(tmp_path, name):
    check_host(tmp_path, tc.BEAGLE_CASES[name]())


def test_the_host_parser_has_atof32s_bits_on_random_accepted_tokens(tmp_path):
    tokens = tc.contract_tokens(100_000, tc.CONTRACT_SEED)
    assert all(tc.device_takes(t) for t in tokens)
    assert tokens[:3000] == tc.contract_tokens(3000, tc.CONTRACT_SEED)                           # seeded: a prefix of the GPU case's tokens
    check_host(tmp_path, tc.tokens_case(tokens, n=100))
    # the generator reaches what it claims: every length, the point at every position, the whole range of net powers, both letters
    assert {len(t) for t in tokens} == set(range(1, 17))
    assert {(len(t.lstrip(b"+-").split(b"e")[0].split(b"E")[0]), t.lstrip(b"+-").find(b".")) for t in tokens if b"." in t} >= {
        (d + 1, p) for d in range(1, 15) for p in range(d + 1)}
    nets = set()
    for t in tokens:
        whole, frac, ex = tc._TAKEN.fullmatch(t).groups()
        nets.add(int(ex or 0) - len(frac))
    assert nets == set(range(-22, 23))
    want = tc.atof32_many(tokens)
    assert np.abs(want).max() > 1e34 and 0 < np.abs(want[want != 0]).min() < 1e-21
    assert any(b"e" in t for t in tokens) and any(b"E" in t for t in tokens)


def test_ties_are_ties_and_atof32_rounds_them_exactly():
    triples = tc.tie_triples()
    assert len(triples) > 300 and len({k for *_, k in triples}) > 30
    assert {b"16777217", b"16777219", b"33554434", b"8388608.5", b"8192.00048828125", b"16384.0009765625"} <= {t for _, t, _, _, _ in triples}
    for below, tie, above, mant, k in triples:
        lo, hi = Fraction(mant) * Fraction(2) ** (k + 1), Fraction(mant + 1) * Fraction(2) ** (k + 1)
        assert Fraction(tie.decode()) * 2 == lo + hi and lo < Fraction(below.decode()) < Fraction(tie.decode()) < Fraction(above.decode()) < hi
        even = lo if mant % 2 == 0 else hi
        for t, want in ((below, lo), (tie, even), (above, hi)):
            assert tc.device_takes(t), t
            for sign, s in ((1, t), (-1, b"-" + t)):
                exact = np.float32(float(Fraction(s.decode())))                                # Fraction -> float is correctly rounded
                assert tc.atof32(s) == exact == np.float32(float(sign * want)), s
                assert float(exact) == sign * want                                             # the float32 is that neighbour exactly


def test_every_997th_f6_token_and_one_decade_of_them(tmp_path):
    for k in range(0, 10_000_000, 997):
        t = tc.f6_token(k)
        assert len(t) == 8 and bits(tc.atof32(t)) == bits(np.float32(float(t))) == bits(np.float32(k / 1e6))
    text, want = tc.f6_decade(7)
    assert want.shape == (1000, 1000) and np.array_equal(np.sort((want.astype(np.float64) * 1e6).round().astype(np.int64).ravel()),
                                                         np.arange(7_000_000, 8_000_000))
    rows, _, _ = host_rows(tmp_path, text)
    assert rows.tobytes() == want.tobytes()
    line = text.split(b"\n")[1].split(b"\t")
    assert tc.atof32_many(line[3::3]).tobytes() == want[0, 0::2].tobytes() and tc.atof32_many(line[4::3]).tobytes() == want[0, 1::2].tobytes()


def test_device_takes_is_the_documented_grammar():
    takes = [b"1e-3", b"+0.5", b"-0.25", b".5", b"5.", b"1E2", b"0.000001", b"1.5e-003", b"00.12345", b"123456789012345", b"1e22", b"2.5E-21", b"0",
             b"0.00000000000001", b"0000000000000000", b"1.e5", b"-0", b"123456789012345.", b"1000000000000000"[:15], b"1e022"]
    leaves = [b"0.1234567890123456789", b"nan", b"inf", b"123456789012345678", b"0x1p-2", b"1e", b"0.5abc", b"-.", b"1e400", b"1e-30", b"2.5E-22",
              b"0.33333333333333333", b"0.0000000000000001", b"", b".", b"+", b"1..", b"+-1", b"e5", b"1e+", b"1e0001", b"1e23", b"1000000000000000",
              b"12345678901234567", b"\x0b1", b"1\x00", b"0.0e999"]
    assert all(tc.device_takes(t) for t in takes) and not any(tc.device_takes(t) for t in leaves)
    assert [tc.depth_takes(t) for t in (b"0", b"255", b"007", b"256", b"0007", b"+7", b"", b"1x", b"\xb2")] == [True, True, True] + [False] * 6


@pytest.mark.parametrize("length", tc.ALIGN_LENGTHS)
def test_alignment_files_cover_every_offset_length_and_boundary_position(length):
    case = tc.alignment_case(length)
    a, b = tc.file_spans(case.lines, case.n)
    assert set((b - a).tolist()) == {length}
    assert min(len(x) for x in case.lines) > 2 * tc.STEP                     # every line passes two steps wherever it begins
    assert sorted(len(x.split(b"\t")[0]) for x in case.lines) == list(range(len(case.lines[0].split(b"\t")[0]), len(case.lines[0].split(b"\t")[0]) + 1040))
    for offset in range(16):
        assert tc.Coverage(offset, a, b).missing([length]) == [], offset
    assert case.flagged == (1040 if length > 16 else 0)


def loadtxt(text, skip=0):
    return np.atleast_2d(np.loadtxt(io.StringIO(text.decode("latin-1")), dtype=np.int32, skiprows=skip))


def test_depth_files_cover_every_form_offset_split_and_strip_position(tmp_path):
    case = tc.depth_forms_case()
    assert np.array_equal(loadtxt(case.text), case.want) and case.want.shape == (1040, 366)
    assert sorted(set(case.lines[0].split())) == sorted(tc.DEPTH_FORMS) and all(tc.depth_takes(t) for t in tc.DEPTH_FORMS)
    assert [len(x) - len(x.lstrip(b" ")) for x in case.lines] == list(range(1040))
    a, b = tc.file_spans(case.lines)
    form = np.array([tc.DEPTH_FORMS.index(t) for x in case.lines for t in x.split()])
    for offset in range(16):
        assert len(set((form * 16 + (a + offset) % 16).tolist())) == 16 * len(tc.DEPTH_FORMS), offset       # every form at every byte of a word
        cov = tc.Coverage(offset, a, b)
        for n in (1, 2, 3):                                                   # a token of every width begins at every byte around the step
            assert {d for w, d in ((x // 64, x % 64) for x in cov.first) if w == n} >= set(range(16 - n + 1, 18)), (offset, n)
    for n in (257, 513):
        case = tc.depth_strip_case(n)
        assert np.array_equal(loadtxt(case.text), case.want)
        starts = tc.strip_starts(case.lines)
        assert len(starts) == 1040 * ((n - 1) // tc.STRIP)
        for offset in range(16):                                              # individual 256 (and 512) begins at every byte of a step:
            assert set(((starts + offset) % tc.STEP).tolist()) == set(range(tc.STEP)), (n, offset)       # the first, the last, ...
    for m in (63, 64, 65, 127, 129):
        assert tc.DEPTH_CASES["tile_%d" % m]().want.shape == (m, 514)


def test_depth_cases_as_loadtxt_and_the_host_parser_read_them(tmp_path):
    import warnings
    case = tc.depth_counts_case()
    table = loadtxt(case.text, skip=1).reshape(len(case.lines), case.n, 4)
    assert {(int(a), int(b)) for a, b in case.majmin} == {(a, b) for a in range(4) for b in range(4)}
    assert all(len({*row}) == 4 for row in table.reshape(-1, 4)[:2000])
    assert [len(t) for t in case.lines[0].split()[:4]] == [1, 2, 3, 1]
    for i in range(case.n):
        assert np.array_equal(case.want[:, 2 * i], table[np.arange(len(table)), i, case.majmin[:, 0]])
        assert np.array_equal(case.want[:, 2 * i + 1], table[np.arange(len(table)), i, case.majmin[:, 1]])
    case = tc.depth_flagged_case()
    want = loadtxt(case.text)
    assert want.min() >= 0 and want.max() <= 255
    assert case.flagged == sum(1 for x in case.lines if not all(tc.depth_takes(t) for t in x.split())) == len(case.lines) // 2
    p = tmp_path / "flagged.txt"
    p.write_bytes(case.text)
    _, rows, _ = table_rows(p, 2 * case.n)
    assert np.array_equal(rows, want)
    # "7" behind a vertical tab: white space to np.loadtxt, which reads the 7, but no delimiter and no digit to the host parser,
    # which refuses the line -- the two differ, so the flagged case leaves the token out (refusals are held in
    # test_gpu_depth_ingest.py)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        seen = loadtxt(b"1 \x0b7 3 4\n")
    assert seen.tolist() == [[1, 7, 3, 4]]
    p.write_bytes(b"1 \x0b7 3 4\n")
    with pytest.raises(ValueError, match="not an integer"):
        table_rows(p, 4)
