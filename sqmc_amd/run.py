"""python -m sqmc_amd.run -i <deck>   (or  < deck)

Runs a reference input deck on the GPU path.  run_type `none`: a projector Monte Carlo walk, see
walk_run.py.  run_type `hci`: the deck grammar of read_input
(do_walk.f90:406-574 for hci decks: seeds, run_type, `eps_var eps_pt target_error n_states`,
dump_wf_var, the chem Hamiltonian block of chemistry.f90:119-245, then the namelists
&selected_ci and &hf_det) and the result lines of perform_hci (hci.f90:323, 487, 833-841), so the
shipped decks (C2_v2z_curve/*/i_1sigma_g) run unchanged next to their FCIDUMP and the same
`grep 'Total energy(1)'` post-processing applies.  PT: deterministic, or with `n_mc > 0` and
`eps_pt_big` in &selected_ci the semistochastic scheme of second_order_pt_alias.  `&natorb get_natorbs=t [use_pt=t] /`
(hci.f90:683-745): the 1-RDM of the variational wavefunction (or its lowest-order PT correction) and its natural orbitals by
irrep, printed as the reference prints them; without --rotate-integrals the run stops there, with it the library rotates the
integrals into the natural orbitals (sqmc_gpu_rotate_integrals) and the run writes them as FCIDUMP_eps_var=... for the next HCI
run, where the reference stops too (:745).  `&greens_function get_greens_function=t n_w=... w_min=... w_max=... /` (hci.f90:748-759): the
zeroth-order Green's function of state 1 on the device (sqmc_gpu_hci_greens_function), written as G0_N+1, G0_N-1 and rho into the
working directory, after which the run goes on to the PT stage as the reference does; --greens-signed selects the matrix elements
with their fermionic sign (the reference applies none).  `&selected_ci n_energy_batch=K /` (hci.f90:638-643, 1824-2017): after the
variational stage the wavefunction is truncated to its leading determinants by magnitude in K + 1 steps, each re-diagonalised and
given its PT stage, one `eps_var, eps_pt, ndets, ...` line per truncation for the extrapolation of E_total against the PT correction,
and the run stops there as the reference does; each truncation's Hamiltonian is the principal submatrix of the whole list's, extracted
on the device (sqmc_gpu_spmv_plan_submatrix), or with --extrap-rebuild built from its determinants.  Host-side plumbing: every piece that scales with the number of determinants runs in libsqmc_gpu."""
import argparse
import os
import re
import sys
import time

import numpy as np


def _strip(line):
    return line.split("!")[0] if line.lstrip().startswith("!") else line


def _logical(tok):
    t = tok.strip().strip(".").lower()
    if t[:1] in ("t", "f"):
        return t[0] == "t"
    raise ValueError("not a Fortran logical: " + tok)


def _numbers(line, n):
    """first n list-directed numeric items of a line (Fortran accepts 1.e-4, 1d-4, commas)"""
    out = []
    for tok in re.split(r"[,\s]+", line.strip()):
        try:
            out.append(float(tok.lower().replace("d", "e")))
        except ValueError:
            break
        if len(out) == n:
            break
    if len(out) < n:
        raise ValueError("expected %d numbers in %r" % (n, line))
    return out


def _namelists(text):
    """&name key=value ... /  ->  {name: {key: [values]}} with r*c repeat counts expanded"""
    groups = {}
    for m in re.finditer(r"^\s*&(\w+)(.*?)/", text, re.S | re.M):
        body, d = m.group(2), {}
        for km in re.finditer(r"(\w+)\s*=\s*([^=]*?)(?=\s+\w+\s*=|\s*$)", body.strip(), re.S):
            vals = []
            for tok in re.split(r"[,\s]+", km.group(2).strip()):
                if not tok:
                    continue
                rep, _, v = tok.partition("*") if "*" in tok else ("1", "", tok)
                vals += [v] * int(rep)
            d[km.group(1).lower()] = vals
        groups[m.group(1).lower()] = d
    return groups


def parse_hci_deck(text):
    lines = [l for l in text.splitlines() if l.strip() and not l.lstrip().startswith("!")]
    deck = {}
    # The decks of src/e2e_tests were written for the grammar in which the walk parameters (six lines:
    # nstep..., w_abs_gen..., tau..., reweight..., population control..., proposal_method...) come before
    # run_type, and semistoch/use_exp_proj after dump_wf_var: recognise it by the position of 'hci'.
    if lines[1].split()[0].strip("'\"").lower() != "hci" and len(lines) > 7 and lines[7].split()[0].strip("'\"").lower() == "hci":
        lines = [lines[0]] + lines[7:10] + lines[11:]
    s = re.sub(r"\s+", " ", lines[0].strip())
    digits = "".join(ch for ch in lines[0][:33] if ch.isdigit())           # '(4i4,x,4i4)'
    deck["irand_seed"] = [[int(digits[4 * i:4 * i + 4]) for i in range(4)], [int(digits[16 + 4 * i:20 + 4 * i]) for i in range(4)]]
    deck["run_type"] = lines[1].split()[0].strip("'\"").lower()
    if deck["run_type"] != "hci":
        raise SystemExit("sqmc_amd.run: only run_type hci decks are driven from a deck file (walks: sqmc_amd.host.GpuWalk / the C ABI)")
    ev, ep, te, ns = _numbers(lines[2], 4)
    deck.update(eps_var=ev, eps_pt=ep, target_error=te, n_states=int(ns))
    deck["dump_wf_var"] = _logical(lines[3].split()[0])
    toks = lines[4].replace(",", " ").split()
    deck["hamiltonian_type"], deck["ipr"] = toks[0].strip("'\"").lower(), int(float(toks[1]))
    nl = _namelists("\n".join(lines[5:]))
    sci = nl.get("selected_ci", {})
    deck["eps_var_sched"] = [float(v.lower().replace("d", "e")) for v in sci.get("eps_var_sched", [])]
    deck["n_mc"] = int(float(sci.get("n_mc", ["0"])[0]))
    deck["eps_pt_big"] = float(sci["eps_pt_big"][0].lower().replace("d", "e")) if "eps_pt_big" in sci else 0.0
    deck["n_energy_batch"] = int(float(sci["n_energy_batch"][0])) if "n_energy_batch" in sci else 0      # hci.f90:638
    nat = nl.get("natorb", {})               # hci.f90:683-745
    deck["get_natorbs"] = _logical(nat["get_natorbs"][0]) if "get_natorbs" in nat else False
    deck["use_pt"] = _logical(nat["use_pt"][0]) if "use_pt" in nat else False
    gf = nl.get("greens_function", {})       # hci.f90:748-759; n_w = 20 unless given
    real = lambda v: float(v.lower().replace("d", "e"))
    deck["get_greens_function"] = _logical(gf["get_greens_function"][0]) if "get_greens_function" in gf else False
    deck["n_w"] = int(real(gf["n_w"][0])) if "n_w" in gf else 20
    deck["w_min"] = real(gf["w_min"][0]) if "w_min" in gf else None
    deck["w_max"] = real(gf["w_max"][0]) if "w_max" in gf else None
    if deck["hamiltonian_type"] == "heg":              # read_heg, heg.f90:102-170
        deck["n_dim"] = int(_numbers(lines[5], 1)[0]); deck["r_s"] = _numbers(lines[6], 1)[0]
        ne, nu = _numbers(lines[7], 2)
        deck.update(nelec=int(ne), nup=int(nu), cutoff_radius=_numbers(lines[8], 1)[0])
        return deck
    if deck["hamiltonian_type"] != "chem":
        raise SystemExit("sqmc_amd.run: hamiltonian_type %r decks are not handled here" % deck["hamiltonian_type"])
    ne, nu = _numbers(lines[5], 2)
    deck.update(nelec=int(ne), nup=int(nu), point_group=lines[6].split()[0].strip("'\"").lower(), time_sym=_logical(lines[7].split()[0]))
    deck["z"] = int(_numbers(lines[8], 1)[0])
    deck["norb"] = int(_numbers(lines[9], 1)[0])
    deck["orbital_symmetries"] = [int(x) for x in _numbers(lines[10], deck["norb"])]
    hf = nl.get("hf_det", {})
    deck["hf_symmetry"] = int(hf["hf_symmetry"][0]) if "hf_symmetry" in hf else None
    if "irreps" in hf:
        raise SystemExit("sqmc_amd.run: &hf_det irreps=... (hand-picked occupations) is not handled; use hf_symmetry")
    return deck


def run_hci_heg(deck, out=sys.stdout, pt_on_device=False, pt_diag_update=0):
    """HEG decks: no integral file; result lines as hci.f90 prints them for 'heg' (no state index in the
    older output format the e2e fixtures were produced with; Madelung total, correlation energy)."""
    if deck.get("get_natorbs"):
        raise SystemExit("Natural orbitals only implemented for chem so far")          # hci.f90:684
    if deck.get("get_greens_function"):
        raise SystemExit("sqmc_amd: &greens_function is built for chem only (the reference calls hamiltonian_chem there, hci.f90:3936)")
    if deck.get("n_energy_batch", 0) > 0:
        raise SystemExit("sqmc_amd: &selected_ci n_energy_batch (energies for extrapolation) is built for chem decks only")
    import torch            # noqa: F401
    import sqmc_amd
    from . import host as H
    p = lambda *a: (print(*a, file=out), out.flush())
    sqmc_amd.set_device(0)
    h = H.HegHost(deck["n_dim"], deck["r_s"], deck["nelec"], deck["nup"], deck["cutoff_radius"])
    p("Within cutoff_radius =%10.5f number of spatial orbitals =%4d" % (deck["cutoff_radius"], h.norb))
    g = h.gpu()
    e_hf = g.hamiltonian_batch([h.hf_up], [h.hf_dn], [h.hf_up], [h.hf_dn])[0]
    mad = h.madelung_energy() if deck["n_dim"] == 3 else 0.0
    p("Madelung energy =%10.6f" % mad)
    p("Iteration   0 %8d =%9.2E dets, energy=%16.6f" % (1, 1.0, e_hf))

    def log(msg):
        m = re.match(r"Iteration\s+(\d+) eps1=(\S+) ndets=\s*(\d+).*energy=(.*)", msg)
        p("Iteration%4d %8d =%9.2E dets, energy=%s" % (int(m.group(1)), int(m.group(3)), float(m.group(3)), "".join("%16.6f" % float(x) for x in m.group(4).split())))
    up, dn, wts, energy, hist = H.hci_variational(h, g, deck["eps_var"], eps_sched=tuple(deck["eps_var_sched"]), n_states=deck["n_states"], log=log)
    res = {"ndets": len(up), "hist": hist, "e_hf": float(e_hf), "madelung": mad}
    e0 = float(energy[0])
    if deck["n_mc"] > 0 and deck["eps_pt_big"] > deck["eps_pt"]:
        r = H.hci_pt2_stochastic(h, g, up, dn, wts[:, 0], e0, deck["eps_pt"], deck["eps_pt_big"], deck["n_mc"], deck["target_error"],
                                 seed=deck["irand_seed"][0], log=lambda m: p("\n" + m), on_device=pt_on_device, diag_update=pt_diag_update)
        de, err = r["pt_big"] + r["pt_diff"], r["pt_diff_std_dev"]
        p("\nVariational energy=%s%15.9f" % (" " * 16, e0))
        p("Second-order PT energy lowering=%s%15.9f +-%12.9f (%13.9f%13.9f)" % (" " * 3, de, err, r["pt_big"], r["pt_diff"]))
        p("Total energy=%s%15.9f +-%12.9f" % (" " * 22, e0 + de, err))
        p("Total energy (includ. Madelung)=%s%15.9f +-%12.9f" % (" " * 3, e0 + de + mad, err))
        res.update(pt=de, pt_err=err, pt_big=r["pt_big"], pt_diff=r["pt_diff"], n_samples=len(r["samples"]))
    else:
        de, nconn = H.hci_pt2(h, g, up, dn, wts[:, 0], e0, deck["eps_pt"], diag_update=pt_diag_update)
        p("\nPT_correction, eps_pt, ndets_connected for fully deterministic run=%15.9f%12.4E%12d" % (de, deck["eps_pt"], nconn))
        p("\nVariational energy=%s%15.9f" % (" " * 16, e0))
        p("Second-order PT energy lowering=%s%15.9f" % (" " * 3, de))
        p("Total energy=%s%15.9f" % (" " * 22, e0 + de))
        p("Total energy (includ. Madelung)=%s%15.9f" % (" " * 3, e0 + de + mad))
        res.update(pt=de, n_connected=nconn)
    p("Correlation energy =%s%15.9f" % (" " * 16, e0 + de - e_hf))
    g.close()
    res.update(e_var=e0, e_total=e0 + de)
    return res


NATORB_STOP = "sqmc_amd: rotating the integrals into FCIDUMP.natorb (generate_natorb_integrals, hci.f90:3681-3846) is not built; stopping after the natural orbitals"


def run_natorbs(deck, h, up, dn, wts, energy, p, one_rdm_path=None, natorb_fcidump=None):
    """&natorb get_natorbs = t (hci.f90:683-745): the 1-RDM of the variational wavefunction, or with use_pt its lowest-order PT
    correction, its natural orbitals by irrep, printed as the reference prints them.  natorb_fcidump = None: the run stops there with
    NATORB_STOP.  A path: the second half of generate_natorb_integrals (hci.f90:3681-3846) -- the integrals rotated into the natural
    orbitals on the device, written to that file (which must not exist) between the reference's two lines, and the run stops where
    the reference stops (:745).  The reference's list-directed 'New orbital symmetries:' lines (:3649, :3679) are left out: their
    spacing is the compiler's choice, and a rotation within irreps leaves the symmetries as the deck gives them."""
    from . import host as H
    from ._lib import SqmcGpuError
    n_states = deck["n_states"]
    if deck["use_pt"]:
        p("\nGetting natural orbitals from the lowest-order perturbative correction to the variational 1-RDM")
        eps_big = deck["eps_pt_big"] if deck["eps_pt_big"] > 0 else deck["eps_pt"]            # :688-689
        p("\nComputing 1-RDM to lowest nonzero order in PT\n")
        try:
            rdm, nconn = H.hci_one_rdm(h, up, dn, wts, energies=energy, use_pt=True, eps_pt_big=eps_big)
        except SqmcGpuError as e:
            if "2^31" in str(e) or "out of memory" in str(e).lower():
                raise SystemExit("sqmc_amd: the connected space at eps_pt_big =%11.4E does not fit (%s); the reference would raise eps_pt_big by its "
                                 "connection estimate here (hci.f90:692-703), which is not built: give an explicit, larger eps_pt_big in &selected_ci" % (eps_big, e))
            raise
        p("\nActual ndets_connected in get_1rdm_with_pt%13d =%9.2E" % (nconn, float(nconn)))
        p("\nPT-corrected 1-RDM:")
    else:
        p(" Getting natural orbitals from the variational 1-RDM")
        if n_states > 1:
            p(" Using state-averaged 1-RDM from the lowest%12d states" % n_states)
            for i in range(n_states):
                p(" Computing 1-RDM of state%12d" % (i + 1))
        p("\nComputing 1-RDM")
        rdm = H.hci_one_rdm(h, up, dn, wts[:, :n_states])
        p("\n1-RDM:")
    p(H.format_real_matrix(rdm))
    p("Done generating rdm")
    occ, vec = H.natural_orbitals(rdm, h.orbsym[1:h.norb + 1])
    p("\nEigenvectors of 1RDM:")
    p(H.format_real_matrix(vec))
    p("Eigenvalues of 1RDM:")
    p(H.format_eigenvalues(occ))
    if one_rdm_path:
        np.save(one_rdm_path, rdm)
    res = dict(ndets=len(up), up=up, dn=dn, wts=wts, energy=energy, rdm=rdm, occupations=occ, vectors=vec)
    if natorb_fcidump is None:
        p("\n" + NATORB_STOP)
        return res
    if os.path.exists(natorb_fcidump):               # open(88, file=filename, status='new'), before any work is done
        raise FileExistsError("sqmc_amd: %s exists; the rotated integrals are written to a new file only" % natorb_fcidump)
    p("\nRotating integrals to new natural orbitals")
    g = h.gpu()
    try:
        packed = g.rotate_integrals(vec)
    finally:
        g.close()
    p("Done computing new integrals. Dumping new integrals into file " + natorb_fcidump)
    H.write_natorb_fcidump(natorb_fcidump, h, packed)
    res.update(natorb_integrals=packed, natorb_fcidump=natorb_fcidump)
    return res


def _greens_checks(deck):
    """what stops a run with &greens_function get_greens_function = t before any work is done"""
    from . import host as H
    if deck["w_min"] is None or deck["w_max"] is None:
        raise SystemExit("sqmc_amd: &greens_function needs w_min and w_max")
    if deck["n_w"] < 2:
        raise SystemExit("sqmc_amd: &greens_function n_w =%d; the frequency grid needs two points at least (hci.f90:751 divides by n_w - 1)" % deck["n_w"])
    for name in H.GREENS_HEADERS:                    # open(60, file='G0_N+1', status='new') and its two neighbours
        if os.path.exists(os.path.join(os.getcwd(), name)):
            raise FileExistsError("sqmc_amd: %s exists; the Green's function is written to new files only" % os.path.join(os.getcwd(), name))


def run_greens(deck, h, up, dn, wts, energy, p, signed=False):
    """&greens_function get_greens_function = t (hci.f90:748-759): the reference's three list-directed lines in fixed formats (i12,
    es24.16e3), the Green's function of state 1 on the device, its three files in the working directory"""
    from . import host as H
    w = H.greens_grid(deck["n_w"], deck["w_min"], deck["w_max"])
    p(" About to compute Green's function for%12d frequencies:" % len(w))
    p("".join(H._es24(x) for x in w))
    p(" E_0 =" + H._es24(float(energy[0])))
    gp, gm = H.hci_greens_function(h, up, dn, wts, float(energy[0]), w, fermi_sign=signed)
    H.write_greens_function(os.getcwd(), w, gp, gm)
    return w, gp, gm


def run_extrapolation(deck, h, g, up, dn, wts, p, pt_on_device=False, pt_diag_update=0, rebuild=False):
    """&selected_ci n_energy_batch = K (hci.f90:638-643, energies_for_extrapolation :1824-2017): the reference's lines for the K + 1
    truncations of the variational wavefunction, after which the run stops as there (:2016).  rebuild: every truncation's matrix from
    its determinants instead of the principal submatrix of the whole list's (host.hci_extrapolation_energies reuse_matrix)."""
    from . import host as H
    try:
        H.extrapolation_truncations(len(up), deck["n_energy_batch"])
    except ValueError as e:
        raise SystemExit("sqmc_amd: " + str(e))
    records = H.hci_extrapolation_energies(h, g, up, dn, wts[:, :deck["n_states"]], deck["n_energy_batch"], deck["eps_var"], deck["eps_pt"], eps_pt_big=deck["eps_pt_big"],
                                           n_mc=deck["n_mc"], target_error=deck["target_error"], seed=deck["irand_seed"][0], reuse_matrix=not rebuild,
                                           pt_diag_update=pt_diag_update, log=p, pt_on_device=pt_on_device)
    return dict(ndets=len(up), extrapolation=records)


def run_two_rdm(h, up, dn, wts, energy, p, path):
    """--two-rdm PATH: the spin blocks of the two-body density matrix of every state of the variational wavefunction (host.hci_two_rdm),
    their checks in print, and all of them in one .npz (aa_1, bb_1, ab_1, aa_2, ...: arrays [p, q, r, s])"""
    from math import comb
    from . import host as H
    nelec, saved, rows = h.nup + h.ndn, {}, []
    p("\nComputing 2-RDM of the variational wavefunction in spin blocks aa, bb, ab")
    for i in range(wts.shape[1]):
        d = H.hci_two_rdm(h, up, dn, wts[:, i])
        sf = H.spin_free_two_rdm(d)
        pairs = {"ab": h.nup * h.ndn, "aa": h.nup * (h.nup - 1), "bb": h.ndn * (h.ndn - 1)}      # a block with pairs exists: nelec >= 2
        b0 = next(b for b in ("ab", "aa", "bb") if pairs[b])
        n2 = float(np.einsum("pqpq->", d[b0])) / pairs[b0]
        one = np.einsum("pqrq->rp", sf) / (nelec - 1)          # [p, r] = <a+_r a_p>, the layout of GpuChem.one_rdm
        e2, s2 = H.rdm_energy(h, one, sf), H.s_squared(h, d["ab"], n2)
        p("\n2-RDM of state%4d:" % (i + 1))
        p(" sum c^2 =%18.12f" % n2)
        for b, want, name in (("aa", comb(h.nup, 2), "C(nup,2)"), ("bb", comb(h.ndn, 2), "C(ndn,2)"), ("ab", h.nup * h.ndn, "nup*ndn")):
            tr = float(np.einsum("pqpq->", d[b])) * (1.0 if b == "ab" else 0.5)
            p(" trace %s =%18.12f   %s =%4d" % (b, tr, name, want))
        p(" Energy from the density matrices =%18.9f   Variational energy =%18.9f   difference =%10.2E" % (e2, energy[i], e2 - energy[i]))
        p(" <S^2> =%16.9f" % s2)
        for b in d:
            saved["%s_%d" % (b, i + 1)] = d[b]
        rows.append(dict(norm2=n2, energy=e2, s_squared=s2))
    with open(path, "wb") as f:
        np.savez(f, **saved)
    p("\n2-RDM blocks written to " + path)
    return rows


def run_transition_rdm(h, up, dn, wts, p, path):
    """--transition-rdm PATH: the one- and two-body transition density matrices of every pair of states i < j of the variational
    wavefunction (host.hci_transition_rdms, bra i and ket j), per pair the overlap, <i|H|j> and <i|S^2|j> from the matrices and the
    three largest singular values of the spin-summed one-body matrix in print, and all matrices in one new .npz (one_1_2, aa_1_2,
    bb_1_2, ab_1_2, ...: arrays [p, r] and [p, q, r, s])"""
    from . import host as H
    if os.path.exists(path):                         # before any work is done, as --rotate-integrals
        raise FileExistsError("sqmc_amd: %s exists; the transition density matrices are written to a new file only" % path)
    saved, rows = {}, []
    p("\nComputing transition density matrices between the states of the variational wavefunction")
    g = H.transition_context(h)                      # one context for every pair of states
    pairs = []
    try:
        for i in range(wts.shape[1]):
            for j in range(i + 1, wts.shape[1]):
                pairs.append((i, j) + H.hci_transition_rdms(h, up, dn, wts, i, j, g=g))
    finally:
        g.close()
    for i, j, one, d in pairs:
        ovl = H.transition_overlap(h, one)
        hij, sij = H.rdm_energy(h, one, H.spin_free_two_rdm(d)), H.s_squared(h, d["ab"], ovl)
        sv = H.natural_transition_orbitals(one)[0]
        p("\nTransition density matrices of states%4d and%4d:" % (i + 1, j + 1))
        p(" Overlap =%10.2E" % ovl)
        p(" <i|H|j> from the density matrices =%10.2E" % hij)
        p(" <i|S^2|j> =%10.2E" % sij)
        p(" Largest singular values of the one-body matrix =" + "".join("%14.9f" % x for x in sv[:3]))
        saved["one_%d_%d" % (i + 1, j + 1)] = one
        for b in d:
            saved["%s_%d_%d" % (b, i + 1, j + 1)] = d[b]
        rows.append(dict(states=(i + 1, j + 1), overlap=ovl, h=hij, s_squared=sij, singular_values=[float(x) for x in sv[:3]]))
    with open(path, "xb") as f:
        np.savez(f, **saved)
    p("\nTransition density matrices written to " + path)
    return rows


def run_optimize_orbitals(h, up, dn, wts, energy, p, path, solver="diagonal"):
    """--optimize-orbitals [PATH]: one orbital-optimisation step on the variational wavefunction (host.optimize_orbitals_step; several
    states: their averaged matrices), its figures in print, and the rotated integrals written to PATH, a new file in the format of
    FCIDUMP_eps_var=... (host.write_natorb_fcidump).  solver "newton" (--orbopt-solver): the Newton-CG step on the device's
    Hessian-vector products, with its count of products, why it stopped and the predicted beside the actual change."""
    from . import host as H
    if os.path.exists(path):                         # before any work is done, as --rotate-integrals
        raise FileExistsError("sqmc_amd: %s exists; the rotated integrals are written to a new file only" % path)
    newton = solver == "newton"
    p("\nOrbital optimisation: one %s step from the 1-RDM and the 2-RDM of the variational wavefunction" % ("Newton-CG" if newton else "diagonal-Newton"))
    r = H.optimize_orbitals_step(h, up, dn, wts, solver="newton") if newton else H.optimize_orbitals_step(h, up, dn, wts)
    e_var = float(np.mean(np.asarray(energy, float)[:wts.shape[1]]))
    p(" Energy from the density matrices =%18.9f   Variational energy =%18.9f   difference =%10.2E" % (r["energy_before"], e_var, r["energy_before"] - e_var))
    p(" max|g| =%14.6E   ||g||_2 =%14.6E" % (r["max_gradient"], r["gradient_norm"]))
    if newton:
        p(" Hessian-vector products =%4d   stopped on: %s" % (r["cg_iterations"], r["cg_stop"]))
    p(" max|kappa| =%14.6E   backtracking scale =%12.8f" % (r["max_kappa"], r["scale"]))
    p(" Fixed-coefficient energy after the step =%18.9f   lowering =%10.2E" % (r["energy_after"], r["energy_after"] - r["energy_before"]))
    if newton:
        p(" Predicted change =%10.2E (of the step before backtracking)   actual change =%10.2E" % (r["predicted_change"], r["energy_after"] - r["energy_before"]))
    H.write_natorb_fcidump(path, h, r["integrals"])
    p("Rotated integrals written to " + path)
    out = dict(path=path, rotation=r["rotation"], integrals=r["integrals"], energy_before=r["energy_before"], energy_after=r["energy_after"],
               max_gradient=r["max_gradient"], gradient_norm=r["gradient_norm"], max_kappa=r["max_kappa"], scale=r["scale"])
    if newton:
        out.update(solver="newton", cg_iterations=r["cg_iterations"], cg_stop=r["cg_stop"], predicted_change=r["predicted_change"])
    return out


def run_hci(deck, fcidump="FCIDUMP", out=sys.stdout, pt_on_device=False, pt_diag_update=0, one_rdm_path=None, natorb_fcidump=None, greens_signed=False,
            extrap_rebuild=False, two_rdm_path=None, optimize_orbitals=None, orbopt_solver="diagonal", transition_rdm_path=None):
    """pt_on_device: the samples of the semistochastic PT are evaluated by the library (host.hci_pt2_stochastic on_device);
    pt_diag_update: 0 / 1 / 2, how the PT stage forms H_aa (host.hci_pt2); one_rdm_path: with &natorb get_natorbs = t, also save the
    1-RDM there as .npy; natorb_fcidump: with &natorb get_natorbs = t, rotate the integrals into the natural orbitals and write them
    to this new file (True: the reference's name, FCIDUMP_eps_var=<smallest eps_var>, in the working directory); the result then
    holds natorb_integrals (packed, the host's combine_2) and natorb_fcidump (the path).  None: the run ends on NATORB_STOP.
    greens_signed: with &greens_function get_greens_function = t, fermi_sign = 1 instead of the reference's sums; the result then holds
    greens = (w, G_np1, G_nm1).  extrap_rebuild: with &selected_ci n_energy_batch > 0, see run_extrapolation; the result then holds
    extrapolation, the records of host.hci_extrapolation_energies.  two_rdm_path: after the variational stage, run_two_rdm; the result
    then holds two_rdm, its per-state records.  Without it the output is what it is without this argument.  optimize_orbitals: after
    the variational stage (and run_two_rdm), run_optimize_orbitals writing to this new file (True: FCIDUMP_opt_eps_var=<smallest
    eps_var>); the result then holds optimize_orbitals.  Without it the output is what it is without this argument.  orbopt_solver:
    "diagonal" (the step as it always was) or "newton" (run_optimize_orbitals); only with optimize_orbitals.  transition_rdm_path:
    after the variational stage (and run_two_rdm), run_transition_rdm on every pair of states; the result then holds
    transition_rdm, its per-pair records.  Without it the output is what it is without this argument."""
    if transition_rdm_path and (deck["hamiltonian_type"] == "heg" or deck.get("get_natorbs") or deck.get("n_energy_batch", 0) > 0):
        raise SystemExit("--transition-rdm runs between the variational and the PT stage of a chem deck: not with heg, &natorb get_natorbs or n_energy_batch > 0, which end elsewhere")
    if transition_rdm_path and deck["n_states"] < 2:
        raise SystemExit("--transition-rdm needs two states at least: n_states = %d" % deck["n_states"])
    if transition_rdm_path and deck["nelec"] < 2:
        raise SystemExit("--transition-rdm needs at least two electrons")
    if orbopt_solver not in ("diagonal", "newton"):
        raise SystemExit("--orbopt-solver: diagonal or newton")
    if orbopt_solver != "diagonal" and not optimize_orbitals:
        raise SystemExit("--orbopt-solver chooses the solver of --optimize-orbitals: give that too")
    if optimize_orbitals and (deck["hamiltonian_type"] == "heg" or deck.get("get_natorbs") or deck.get("n_energy_batch", 0) > 0):
        raise SystemExit("--optimize-orbitals runs between the variational and the PT stage of a chem deck: not with heg, &natorb get_natorbs or n_energy_batch > 0, which end elsewhere")
    if optimize_orbitals and deck["nelec"] < 2:
        raise SystemExit("--optimize-orbitals needs at least two electrons")
    if two_rdm_path and (deck["hamiltonian_type"] == "heg" or deck.get("get_natorbs") or deck.get("n_energy_batch", 0) > 0):
        raise SystemExit("--two-rdm runs between the variational and the PT stage of a chem deck: not with heg, &natorb get_natorbs or n_energy_batch > 0, which end elsewhere")
    if two_rdm_path and deck["nelec"] < 2:
        raise SystemExit("--two-rdm needs at least two electrons")
    if deck["hamiltonian_type"] == "heg":
        return run_hci_heg(deck, out, pt_on_device, pt_diag_update)
    want_greens = bool(deck.get("get_greens_function")) and not deck.get("get_natorbs")      # get_natorbs stops first (hci.f90:745)
    if want_greens:
        _greens_checks(deck)
    import torch            # noqa: F401  one libamdhip64 per process
    import sqmc_amd
    from . import host as H
    p = lambda *a: (print(*a, file=out), out.flush())
    sqmc_amd.set_device(0)
    t0 = time.perf_counter()
    h = H.ChemHost(fcidump, deck["nelec"], deck["nup"], deck["point_group"], time_sym=deck["time_sym"], z=deck["z"], hf_symmetry=deck["hf_symmetry"])
    if h.norb != deck["norb"]:
        raise SystemExit("norb of the deck (%d) and of %s (%d) differ" % (deck["norb"], fcidump, h.norb))
    if list(h.orbsym_file[1:]) != deck["orbital_symmetries"]:
        raise SystemExit("orbital_symmetries of the deck and ORBSYM of %s differ" % fcidump)
    n_states, eps_var = deck["n_states"], deck["eps_var"]
    g = h.gpu()
    g.set_hb_tables(*h.hb_tables(g))
    wf = H.wf_filename(min([eps_var] + deck["eps_var_sched"]))
    if os.path.exists(wf):
        p("\nReading variational wavefn from " + wf)
        up, dn, wts, energy = H.read_wf_var(wf, n_states)
    else:
        e_hf = g.hamiltonian_batch([h.hf_up], [h.hf_dn], [h.hf_up], [h.hf_dn])[0]
        sched = deck["eps_var_sched"] or [eps_var]
        p("Iteration   0 eps1=%s ndets=%9d =%9.2E energy=%s" % (_es71(sched[0]), 1, 1.0, "".join("%16.6f" % v for v in [e_hf] + [0.0] * (n_states - 1))))

        def log(msg):                                   # host.hci_variational reports one line per iteration
            m = re.match(r"Iteration\s+(\d+) eps1=(\S+) ndets=\s*(\d+).*energy=(.*)", msg)
            it, eps, nd, en = int(m.group(1)), float(m.group(2)), int(m.group(3)), [float(x) for x in m.group(4).split()]
            p("Iteration%4d eps1=%s ndets=%9d =%9.2E energy=%s" % (it, _es71(eps), nd, float(nd), "".join("%16.6f" % v for v in en)))
        up, dn, wts, energy, hist = H.hci_variational(h, g, eps_var, eps_sched=tuple(deck["eps_var_sched"]), n_states=n_states, log=log)
        if deck["dump_wf_var"]:
            p("\nWriting variational wavefn to " + wf)
            H.write_wf_var(wf, up, dn, wts, energy)
    if deck.get("n_energy_batch", 0) > 0:            # hci.f90:638-643, in front of natural orbitals, Green's function and the PT stage
        try:
            return run_extrapolation(deck, h, g, up, dn, wts, p, pt_on_device, pt_diag_update, extrap_rebuild)
        finally:
            g.close()
    g.close()
    t1 = time.perf_counter()
    if deck.get("get_natorbs"):
        if natorb_fcidump is True:
            natorb_fcidump = H.natorb_fcidump_name(min([eps_var] + deck["eps_var_sched"]))
        return run_natorbs(deck, h, up, dn, wts, energy, p, one_rdm_path, natorb_fcidump)
    two_rdm = None
    if two_rdm_path:
        two_rdm = run_two_rdm(h, up, dn, np.asarray(wts, float).reshape(len(up), -1), energy, p, two_rdm_path)
        t0, t1 = t0 + (time.perf_counter() - t1), time.perf_counter()      # keep the stage out of both times of the last line
    transition = None
    if transition_rdm_path:
        transition = run_transition_rdm(h, up, dn, np.asarray(wts, float).reshape(len(up), -1)[:, :n_states], p, transition_rdm_path)
        t0, t1 = t0 + (time.perf_counter() - t1), time.perf_counter()      # keep the stage out of both times of the last line
    optorb = None
    if optimize_orbitals:
        if optimize_orbitals is True:
            optimize_orbitals = H.optorb_fcidump_name(min([eps_var] + deck["eps_var_sched"]))
        optorb = run_optimize_orbitals(h, up, dn, np.asarray(wts, float).reshape(len(up), -1)[:, :n_states], energy, p, optimize_orbitals, orbopt_solver)
        t0, t1 = t0 + (time.perf_counter() - t1), time.perf_counter()      # keep the stage out of both times of the last line
    greens = run_greens(deck, h, up, dn, wts, energy, p, greens_signed) if want_greens else None
    results = []
    for i in range(n_states):
        if deck["n_mc"] > 0 and deck["eps_pt_big"] > deck["eps_pt"]:
            # semistochastic PT (second_order_pt_alias): deterministic at eps_pt_big + sampled difference; in the determinant basis
            plain, du, dd, dc = h, up, dn, wts[:, i]
            if h.time_sym:
                import copy
                plain = copy.copy(h); plain.time_sym = False
                du, dd, dc = H.time_symmetrized_to_dets(up, dn, wts[:, i], h.z)
            gp = plain.gpu()
            gp.set_hb_tables(*plain.hb_tables(gp))
            try:
                r = H.hci_pt2_stochastic(plain, gp, du, dd, dc, float(energy[i]), deck["eps_pt"], deck["eps_pt_big"], deck["n_mc"], deck["target_error"],
                                         seed=deck["irand_seed"][0], log=lambda m: p("\n" + m), on_device=pt_on_device, diag_update=pt_diag_update)
            finally:
                gp.close()
            de, nconn = r["pt_big"] + r["pt_diff"], r["n_connected_big"]
            p("\nState%4d:" % (i + 1))
            p("Variational energy(%d)=%s%15.9f" % (i + 1, " " * 12, energy[i]))
            p("2nd-order PT energy lowering(%d)=%s%15.9f +-%12.9f (%13.9f%13.9f)" % (i + 1, " " * 2, de, r["pt_diff_std_dev"], r["pt_big"], r["pt_diff"]))
            p("Total energy(%d)=%s%15.9f +-%12.9f" % (i + 1, " " * 18, energy[i] + de, r["pt_diff_std_dev"]))
            results.append((float(energy[i]), float(de), int(nconn)))
            continue
        de, nconn = H.hci_pt2_determinant_basis(h, up, dn, wts[:, i], float(energy[i]), deck["eps_pt"], diag_update=pt_diag_update)
        p("\nState%4d:" % (i + 1))
        p("Variational energy(%d)=%s%15.9f" % (i + 1, " " * 12, energy[i]))
        p("2nd-order PT energy lowering(%d)=%s%15.9f" % (i + 1, " " * 2, de))
        p("Total energy(%d)=%s%15.9f" % (i + 1, " " * 18, energy[i] + de))
        p("eps_var, eps_pt, ndets, ndets_connected(total), Variational, PT_actv, PT_full, Total Energies(%d)=%8.1E%8.1E%9d%11d%16.9f%15.9f%15.9f%16.9f"
          % (i + 1, eps_var, deck["eps_pt"], len(up), nconn, energy[i], de, de, energy[i] + de))
        results.append((float(energy[i]), float(de), int(nconn)))
    p("\nsqmc_amd: variational stage %.2f s, PT stage %.2f s on the GPU path" % (t1 - t0, time.perf_counter() - t1))
    res = dict(ndets=len(up), states=results)
    if greens is not None:
        res["greens"] = greens
    if two_rdm is not None:
        res["two_rdm"] = two_rdm
    if transition is not None:
        res["transition_rdm"] = transition
    if optorb is not None:
        res["optimize_orbitals"] = optorb
    return res


def _es71(x):
    """Fortran es7.1e1"""
    m, e = ("%.1e" % x).split("e")
    return "%sE%s%d" % (m, "-" if int(e) < 0 else "+", abs(int(e)))


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m sqmc_amd.run", description=__doc__.split("\n\n")[0])
    ap.add_argument("-i", "--input", default=None, help="deck file (default: stdin)")
    ap.add_argument("--fcidump", default="FCIDUMP", help="integral file (the reference reads ./FCIDUMP)")
    ap.add_argument("--walkalize", default=None, help="walk decks: write the per-step record of unit 1 (step, 1/rew_fac_inv, w_abs_gen, e_gen, nwalk) to this file")
    for name, what in (("psit-con", "C(T): Psi_T connections with local-energy pieces (psit_con_in/out_file, semistoch.f90:86-126)"),
                       ("dtm-elems", "the deterministic space and its Hamiltonian (dtm_elems_in/out_file, do_walk.f90:898-1010)")):
        ap.add_argument("--%s-in" % name, default=None, help="walk decks: read %s from this file instead of building it" % what)
        ap.add_argument("--%s-out" % name, default=None, help="walk decks: write %s to this file" % what)
    ap.add_argument("--pt-on-device", action="store_true", help="HCI decks with n_mc > 0: evaluate every sample of the semistochastic PT in the library "
                    "(sqmc_gpu_hci_pt2_stochastic_sample) instead of numpy on the raw connection list")
    ap.add_argument("--pt-diag-update", type=int, choices=(0, 1, 2), default=0, help="HCI decks: H_aa of the PT stage from scratch (0, default), by the O(N) update "
                    "of get_new_diag_elem on one lane (1) or by 16-lane groups (2); with n_mc > 0 it needs --pt-on-device")
    ap.add_argument("--spawn-histograms", action="store_true", help="walk decks: keep and print the reference's histograms of abs(weight_j)/tau = |H_ij|/p "
                    "(off_diag_histograms, do_walk.f90:3295-3311) and, at ipr >= 1, its max / min weight-ratio line; steps run un-pipelined")
    ap.add_argument("--one-rdm", default=None, metavar="PATH", help="HCI decks with &natorb get_natorbs = t: also save the (norb, norb) 1-RDM as a .npy file")
    ap.add_argument("--rotate-integrals", nargs="?", const=True, default=None, metavar="PATH", help="HCI decks with &natorb get_natorbs = t: rotate the integrals "
                    "into the natural orbitals on the device and write them to PATH, a new file (default: FCIDUMP_eps_var=<smallest eps_var>, the reference's name)")
    ap.add_argument("--greens-signed", action="store_true", help="HCI decks with &greens_function get_greens_function = t: the matrix elements with their "
                    "fermionic sign (fermi_sign = 1) instead of the reference's sums, which apply none")
    ap.add_argument("--extrap-rebuild", action="store_true", help="HCI decks with &selected_ci n_energy_batch > 0: build every truncation's Hamiltonian from its "
                    "determinants instead of extracting it from the whole list's on the device (the yardstick; the numbers are the same)")
    ap.add_argument("--two-rdm", default=None, metavar="PATH", help="chem HCI decks: after the variational stage compute the two-body density matrix of every "
                    "state in spin blocks on the device, print its traces, the energy it gives and <S^2>, and save the blocks to PATH (.npz); refused with heg decks, "
                    "&natorb get_natorbs and n_energy_batch > 0, whose runs end elsewhere")
    ap.add_argument("--optimize-orbitals", nargs="?", const=True, default=None, metavar="PATH", help="chem HCI decks: after the variational stage take one "
                    "orbital-optimisation step from the 1-RDM and 2-RDM on the device (gradient, diagonal Hessian, backtracking on the fixed-coefficient energy), "
                    "print its figures and write the rotated integrals to PATH, a new file (default: FCIDUMP_opt_eps_var=<smallest eps_var>); refused with heg "
                    "decks, &natorb get_natorbs and n_energy_batch > 0, whose runs end elsewhere")
    ap.add_argument("--orbopt-solver", choices=("diagonal", "newton"), default="diagonal", help="with --optimize-orbitals: the diagonal-Newton step (default) or "
                    "a line-search Newton-CG step on the device's orbital Hessian-vector products; prints the number of products, why the solver stopped and "
                    "the predicted beside the actual change")
    ap.add_argument("--transition-rdm", default=None, metavar="PATH", help="chem HCI decks with n_states >= 2: after the variational stage compute the one- and "
                    "two-body transition density matrices of every pair of states on the device, print the overlap, <i|H|j> and <i|S^2|j> they give and the "
                    "largest singular values of the one-body matrix, and save them to PATH, a new .npz; refused with n_states = 1, heg decks, &natorb "
                    "get_natorbs and n_energy_batch > 0")
    a = ap.parse_args(argv)
    text = open(a.input).read() if a.input else sys.stdin.read()
    lines = [l for l in text.splitlines() if l.strip() and not l.lstrip().startswith("!")]
    run_type = lines[1].split()[0].strip("'\"").lower() if len(lines) > 1 else ""
    if run_type in ("none", "no_fixed_node"):          # a projector walk: the grammar of read_input for run_type /= hci
        from .walk_run import parse_walk_deck, run_walk
        return run_walk(parse_walk_deck(text), a.fcidump, walkalize=a.walkalize, psit_con_in=a.psit_con_in, psit_con_out=a.psit_con_out,
                        dtm_elems_in=a.dtm_elems_in, dtm_elems_out=a.dtm_elems_out, spawn_histograms=a.spawn_histograms)
    deck = parse_hci_deck(text)
    return run_hci(deck, a.fcidump, pt_on_device=a.pt_on_device, pt_diag_update=a.pt_diag_update, one_rdm_path=a.one_rdm, natorb_fcidump=a.rotate_integrals,
                   greens_signed=a.greens_signed, extrap_rebuild=a.extrap_rebuild, two_rdm_path=a.two_rdm, optimize_orbitals=a.optimize_orbitals, orbopt_solver=a.orbopt_solver,
                   transition_rdm_path=a.transition_rdm)


if __name__ == "__main__":
    main()
