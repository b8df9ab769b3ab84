"""host.write_natorb_fcidump on synthetic packed arrays: the file generate_natorb_integrals writes (hci.f90:3794-3841), character for
character, and that the project's readers read it back.  No GPU: a ChemHost without hf_symmetry is built on the host alone."""
import re

import numpy as np
import pytest

import proposal_checker as PC
import rotate_checker as RC
from sqmc_amd import host as H

NORB = 5
ORBSYM = [1, 2, 1, 2, 1]


def _source_fcidump(path, commas=True):
    """one-body energies that put the file's orbitals in the order 1, 4, 2, 5, 3 (the occupied one first, then by energy)"""
    with open(path, "w") as f:
        f.write(" &FCI NORB=%d,NELEC=2,MS2=0,\n" % NORB)
        f.write("  ORBSYM=" + (",".join(map(str, ORBSYM)) + "," if commas else "".join("%3d" % s for s in ORBSYM)) + "\n  ISYM=1\n &END\n")
        for k, e in enumerate([-2.0, 0.1, 0.7, -0.5, 0.4]):
            f.write("%.17e %d %d 0 0\n" % (e, k + 1, k + 1))
        f.write("%.17e 1 1 1 1\n" % 0.25)
        f.write("%.17e 0 0 0 0\n" % 1.5)


@pytest.fixture()
def host(tmp_path):
    p = tmp_path / "SRC"
    _source_fcidump(p)
    h = H.ChemHost(str(p), 2, 1, "cs")
    assert list(h.orb_order[1:NORB + 1]) == [1, 4, 2, 5, 3]
    return h


def _synthetic(h, seed=0):
    """a packed array with every addressed slot set: values over twelve decades of both signs, and the threshold's neighbours"""
    rng = np.random.default_rng(seed)
    v = np.zeros(len(h.integrals))
    a2, a1, ac = RC.addresses(NORB, h.combine_2)
    v[a2] = rng.choice([-1.0, 1.0], len(a2)) * 10.0 ** rng.uniform(-9.5, 2.5, len(a2))
    v[a2[:6]] = [1e-8, -1e-8, 1.0000001e-8, -1.0000001e-8, 0.0, 9.9999e-9]
    for p in range(NORB):
        for q in range(p + 1):
            v[a1[p, q]] = rng.uniform(-3, 3)
    v[a1[2, 1]] = 1e-8
    v[a1[3, 0]] = -5e-9
    v[ac] = -12.345678901234567
    return v


def _expected_records(h, v):
    """the reference's loops, with this test's own addressing"""
    o, c2, n1 = h.orb_order, h.combine_2, NORB + 1
    ix = lambda i, j, k, l: int(RC.packed_index(c2, np.array(i), np.array(j), np.array(k), np.array(l)))
    out = []
    for p in range(1, n1):
        for q in range(1, p + 1):
            for r in range(1, p + 1):
                for s in range(1, r + 1):
                    if p == r and q < s:
                        continue
                    x = v[ix(p, q, r, s)]
                    if abs(x) > 1e-8:
                        out.append((x, int(o[p]), int(o[q]), int(o[r]), int(o[s])))
    for p in range(1, n1):
        for q in range(1, p + 1):
            x = v[ix(p, q, n1, n1)]
            if abs(x) > 1e-8:
                out.append((x, int(o[p]), int(o[q]), 0, 0))
    out.append((v[ix(n1, n1, n1, n1)], 0, 0, 0, 0))
    return out


def test_header_records_order_and_threshold(host, tmp_path):
    v = _synthetic(host)
    path = tmp_path / "FCIDUMP_new"
    H.write_natorb_fcidump(str(path), host, v)
    lines = path.read_text().split("\n")
    assert lines[-1] == "" and lines[:4] == ["&FCI NORB=    5, NELEC=    2, MS2=0", "ORBSYM=  1  2  1  2  1", "ISYM=1", "&END"]
    recs = lines[4:-1]
    want = _expected_records(host, v)
    assert len(recs) == len(want) > 100
    fmt = re.compile(r"^[ -]\d\.\d{12}E[+-]\d\d( {3}\d| {2}\d\d| \d{3}|\d{4}){4}$")          # (es19.12e2,4i4)
    for line, (x, a, b, c, d) in zip(recs, want):
        assert fmt.match(line) and len(line) == 35, line
        assert [int(line[19 + 4 * k:23 + 4 * k]) for k in range(4)] == [a, b, c, d]            # the loop order, record by record
        assert float(line[:19]) == float("%.12E" % x)
    assert recs[-1] == "-1.234567890123E+01   0   0   0   0"
    # nothing at or below the threshold, everything above it
    written = [abs(float(l[:19])) for l in recs[:-1]]
    assert min(written) > 1e-8
    a2, a1, ac = RC.addresses(NORB, host.combine_2)
    n_above = int((np.abs(v[a2]) > 1e-8).sum()) + sum(abs(v[a1[p, q]]) > 1e-8 for p in range(NORB) for q in range(p + 1))
    assert len(recs) - 1 == n_above and n_above < len(a2) + NORB * (NORB + 1) // 2 - 4


def test_refuses_to_overwrite(host, tmp_path):
    path = tmp_path / "F"
    H.write_natorb_fcidump(str(path), host, _synthetic(host))
    before = path.read_bytes()
    with pytest.raises(FileExistsError):
        H.write_natorb_fcidump(str(path), host, _synthetic(host, seed=1))
    assert path.read_bytes() == before
    with pytest.raises(ValueError):
        H.write_natorb_fcidump(str(tmp_path / "G"), host, np.zeros(3))


def test_reads_back_through_both_readers(host, tmp_path):
    v = _synthetic(host)
    path = tmp_path / "F"
    H.write_natorb_fcidump(str(path), host, v)
    want = _expected_records(host, v)
    norb, orbsym, vals, idx = H.read_fcidump(str(path))
    assert norb == NORB and orbsym == ORBSYM                                                   # an ORBSYM line without commas
    assert len(vals) == len(want)
    for x, lab, (w, a, b, c, d) in zip(vals, idx.tolist(), want):
        assert lab == [a, b, c, d] and x == float("%.12E" % w)
    n2, one, two, core = PC.read_fcidump(str(path))
    assert n2 == NORB and core == float("%.12E" % want[-1][0])
    n_one = n_two = 0
    for w, a, b, c, d in want[:-1]:
        if c == 0:
            assert one[(max(a, b), min(a, b))] == float("%.12E" % w); n_one += 1
        else:
            assert two[PC._eri_key(a, b, c, d)] == float("%.12E" % w); n_two += 1
    assert len(one) == n_one and len(two) == n_two
    # and a host built from the file holds the written values at its own addresses (the new file's orbital order is its own)
    h2 = H.ChemHost(str(path), 2, 1, "cs")
    assert list(h2.orbsym_file[1:]) == ORBSYM
    inv = {int(h2.orb_order[i]): i for i in range(1, NORB + 1)}
    for w, a, b, c, d in want[:-1]:
        i = [inv[x] if x else NORB + 1 for x in (a, b, c, d)]
        assert h2.integrals[int(RC.packed_index(h2.combine_2, *map(np.array, i)))] == float("%.12E" % w)


def test_file_name():
    assert H.natorb_fcidump_name(5e-3) == "FCIDUMP_eps_var=5.00E-3"
    assert H.natorb_fcidump_name(1e-4) == "FCIDUMP_eps_var=1.00E-4"
    assert H.natorb_fcidump_name(2e-5) == "FCIDUMP_eps_var=2.00E-5"


def test_orbsym_with_and_without_commas(tmp_path):
    a, b = tmp_path / "A", tmp_path / "B"
    _source_fcidump(a, commas=True)
    _source_fcidump(b, commas=False)
    ra, rb = H.read_fcidump(str(a)), H.read_fcidump(str(b))
    assert ra[0] == rb[0] == NORB and ra[1] == rb[1] == ORBSYM
    assert np.array_equal(ra[2], rb[2]) and np.array_equal(ra[3], rb[3])
    golden = H.read_fcidump(str(__import__("pathlib").Path(__file__).parent / "golden" / "C2_r1.24253_FCIDUMP"))
    assert golden[0] == 26 and len(golden[1]) == 26 and set(golden[1]) <= set(range(1, 9))


def test_with_integrals_keeps_the_order_and_drops_the_heat_bath_table(host):
    host.hb = ("stale",)
    v = _synthetic(host)
    h2 = host.with_integrals(v)
    assert h2 is not host and np.array_equal(h2.integrals, v) and h2.integrals is not v and not hasattr(h2, "hb")
    assert host.hb == ("stale",) and not np.array_equal(host.integrals, v)
    assert h2.combine_2 is host.combine_2 and h2.orb_order is host.orb_order and h2.orbsym is host.orbsym
    assert (h2.hf_up, h2.hf_dn) == (host.hf_up, host.hf_dn)
    with pytest.raises(ValueError):
        host.with_integrals(v[:-1])
