"""ctypes binding of include/sqmc_gpu.h (the same entry points the Fortran iso_c_binding
module sqmc_amd/fortran/sqmc_gpu_mod.f90 binds)."""
import ctypes as C
import os
import subprocess
import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)
def _lib_path():
    """the library's file: builds with extra flags (SQMC_EXTRA_CFLAGS: the instrumented builds of tools/*_prof.py) get a name of their own, so
    that they can neither overwrite the product's library nor be mistaken for it by the staleness check"""
    extra = os.environ.get("SQMC_EXTRA_CFLAGS", "").split()
    if not extra:
        return os.path.join(_HERE, "libsqmc_gpu.so")
    import hashlib
    return os.path.join(_HERE, "libsqmc_gpu_%s.so" % hashlib.sha1(" ".join(extra).encode()).hexdigest()[:10])


LIB_PATH = _lib_path()
RNG_REPLAY, RNG_COUNTER = 0, 1
_LIB = None

EXPORTS = [
    "sqmc_gpu_set_device", "sqmc_gpu_init_chem", "sqmc_gpu_init_heg", "sqmc_gpu_init_hubbard", "sqmc_gpu_init_hubbardk", "sqmc_gpu_set_hubbardk_space_sym", "sqmc_gpu_hubbardk_sym_images", "sqmc_gpu_finalize", "sqmc_gpu_last_error", "sqmc_gpu_set_hb_tables", "sqmc_gpu_set_heatbath_tables", "sqmc_gpu_setup_efficient_heatbath", "sqmc_gpu_get_heatbath_tables", "sqmc_gpu_propose_heatbath_batch", "sqmc_gpu_setup_cauchy_schwarz", "sqmc_gpu_propose_cauchy_schwarz_batch", "sqmc_gpu_set_projector",
    "sqmc_gpu_scale_projector", "sqmc_gpu_set_ct_table", "sqmc_gpu_set_hf_to_psit", "sqmc_gpu_set_hf_to_psit_shard", "sqmc_gpu_upload_walkers", "sqmc_gpu_num_walkers",
    "sqmc_gpu_download_walkers", "sqmc_gpu_step", "sqmc_gpu_run", "sqmc_gpu_annihilate", "sqmc_gpu_det_owner", "sqmc_gpu_set_owner_hash", "sqmc_gpu_shard_config",
    "sqmc_gpu_shard_begin", "sqmc_gpu_shard_pack", "sqmc_gpu_shard_finish", "sqmc_gpu_shard_finish_psit", "sqmc_gpu_comm_unique_id", "sqmc_gpu_comm_init", "sqmc_gpu_comm_size",
    "sqmc_gpu_shard_step", "sqmc_gpu_shard_run", "sqmc_gpu_shard_time_split", "sqmc_gpu_get_rng", "sqmc_gpu_set_rng", "sqmc_gpu_tail_stats", "sqmc_gpu_last_tail", "sqmc_gpu_slowest_steps", "sqmc_gpu_set_chained_runs", "sqmc_gpu_spmv_prepare", "sqmc_gpu_davidson",
    "sqmc_gpu_spmv_apply", "sqmc_gpu_spmv_free", "sqmc_gpu_spmv_plan_submatrix", "sqmc_gpu_build_spmv_plan", "sqmc_gpu_spmv_sym_upper", "sqmc_gpu_hamiltonian_batch",
    "sqmc_gpu_propose_batch", "sqmc_gpu_hamiltonian_chem_batch", "sqmc_gpu_build_sparse_ham", "sqmc_gpu_hci_connections", "sqmc_gpu_hci_connections_slice", "sqmc_gpu_hci_pt2", "sqmc_gpu_hci_pt2_stochastic_prepare", "sqmc_gpu_hci_pt2_stochastic_sample", "sqmc_gpu_hci_pt2_stochastic_stats", "sqmc_gpu_hci_pt2_stochastic_free", "sqmc_gpu_hci_set_active_space", "sqmc_gpu_diag_update_batch", "sqmc_gpu_hci_set_diag_update", "sqmc_gpu_hci_connections_record", "sqmc_gpu_hci_1rdm", "sqmc_gpu_hci_1rdm_pt", "sqmc_gpu_hci_2rdm", "sqmc_gpu_hci_1tdm", "sqmc_gpu_hci_2tdm", "sqmc_gpu_rotate_integrals", "sqmc_gpu_orbital_gradient", "sqmc_gpu_one_index_transform", "sqmc_gpu_orbopt_prepare", "sqmc_gpu_orbopt_gradient", "sqmc_gpu_orbopt_hessian_vector", "sqmc_gpu_orbopt_free", "sqmc_gpu_hci_greens_function", "sqmc_gpu_free", "sqmc_gpu_set_timing", "sqmc_gpu_get_timing",
    "sqmc_gpu_set_spawn_diagnostics", "sqmc_gpu_reset_spawn_diagnostics", "sqmc_gpu_get_spawn_diagnostics", "sqmc_gpu_debug_bucket_boundaries",
]


_ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int64, C.c_void_p)      # sqmc_allreduce_fn


class SqmcGpuError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("libsqmc_gpu status %d: %s" % (code, msg))
        self.code = code


def build_library(force=False):
    """hipcc cross-compiles for gfx950 without a GPU present."""
    csrc = os.path.join(_HERE, "csrc")
    # four translation units: sqmc_gpu.hip includes every .h / .inc of csrc/ textually but rdm2_kernels.h, orbopt_kernels.h and
    # tdm_kernels.h, which rdm2_device.hip, orbopt_device.hip and tdm_device.hip compile into code objects of their own
    units = [os.path.join(csrc, f) for f in ("sqmc_gpu.hip", "rdm2_device.hip", "orbopt_device.hip", "tdm_device.hip")]
    src = units + sorted(os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith((".h", ".inc"))) \
        + [os.path.join(_ROOT, "include", "sqmc_gpu.h")]
    if not force and os.path.exists(LIB_PATH) and all(os.path.getmtime(LIB_PATH) >= os.path.getmtime(s) for s in src):
        return LIB_PATH
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-Wno-unused-value",
           "-I" + os.path.join(_ROOT, "include")] + os.environ.get("SQMC_EXTRA_CFLAGS", "").split() + units + ["-o", LIB_PATH]
    subprocess.check_call(cmd)
    return LIB_PATH


class ChemCfg(C.Structure):
    _fields_ = [("norb", C.c_int32), ("nup", C.c_int32), ("ndn", C.c_int32), ("n_core_orb", C.c_int32),
                ("time_sym", C.c_int32), ("z", C.c_int32), ("n_group", C.c_int32),
                ("product_table", C.c_void_p), ("orbital_symmetries", C.c_void_p), ("combine_2", C.c_void_p),
                ("n_integrals", C.c_int64), ("integrals", C.c_void_p), ("rng_mode", C.c_int32),
                ("irand_seed", C.c_int32 * 4), ("mwalk", C.c_int64)]


class HegCfg(C.Structure):
    _fields_ = [("n_dim", C.c_int32), ("norb", C.c_int32), ("nup", C.c_int32), ("ndn", C.c_int32), ("length_cell", C.c_double),
                ("k_vectors", C.c_void_p), ("rng_mode", C.c_int32), ("irand_seed", C.c_int32 * 4), ("mwalk", C.c_int64)]


class HubbardCfg(C.Structure):
    _fields_ = [("l_x", C.c_int32), ("l_y", C.c_int32), ("pbc", C.c_int32), ("nup", C.c_int32), ("ndn", C.c_int32),
                ("t", C.c_double), ("U", C.c_double), ("rng_mode", C.c_int32), ("irand_seed", C.c_int32 * 4), ("mwalk", C.c_int64)]


class HubbardKCfg(C.Structure):
    _fields_ = [("l_x", C.c_int32), ("l_y", C.c_int32), ("nup", C.c_int32), ("ndn", C.c_int32), ("t", C.c_double), ("U", C.c_double),
                ("k_vectors", C.c_void_p), ("k_energies", C.c_void_p), ("rng_mode", C.c_int32), ("irand_seed", C.c_int32 * 4), ("mwalk", C.c_int64)]


class StepParams(C.Structure):
    _fields_ = [("tau", C.c_double), ("e_trial", C.c_double), ("reweight_factor_inv", C.c_double), ("r_initiator", C.c_double),
                ("min_wt", C.c_double), ("always_spawn_cutoff_wt", C.c_double), ("initiator_power", C.c_int32),
                ("initiator_min_distance", C.c_int32), ("c_t_initiator", C.c_int32), ("semistochastic", C.c_int32),
                ("reached_w_abs_gen", C.c_int32), ("reserved", C.c_int32)]


class PopCtl(C.Structure):
    _fields_ = [("tau_sav", C.c_double), ("tau", C.c_double), ("tau_prev", C.c_double), ("e_trial", C.c_double), ("e_est", C.c_double),
                ("w_abs_gen_target", C.c_double), ("w_abs_gen", C.c_double), ("r_initiator_sav", C.c_double), ("r_initiator", C.c_double),
                ("initiator_rescale_power", C.c_double), ("population_control_exponent", C.c_double), ("reweight_factor_inv", C.c_double),
                ("reweight_factor_inv_max", C.c_double), ("e_num_cum", C.c_double), ("e_den_cum", C.c_double), ("min_wt", C.c_double),
                ("always_spawn_cutoff_wt", C.c_double), ("reached_w_abs_gen", C.c_int32), ("initiator_power", C.c_int32),
                ("initiator_min_distance", C.c_int32), ("c_t_initiator", C.c_int32), ("semistochastic", C.c_int32), ("reserved", C.c_int32),
                ("istep", C.c_int64), ("n_equil", C.c_int64)]


def load_library():
    """Loads the in-tree HIP library; raises if it is missing (no fallback path exists)."""
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise SqmcGpuError(-2, "sqmc_amd/libsqmc_gpu.so is not built: run __graft_entry__.build()")
        L = C.CDLL(LIB_PATH)
        L.sqmc_gpu_last_error.restype = C.c_char_p
        for name in EXPORTS:
            getattr(L, name)   # AttributeError if the ABI lost a symbol
        L.sqmc_gpu_scale_projector.argtypes = [C.c_void_p, C.c_double]
        L.sqmc_gpu_set_hb_tables.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_double]
        L.sqmc_gpu_set_projector.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]
        L.sqmc_gpu_set_ct_table.argtypes = [C.c_void_p, C.c_int64] + [C.c_void_p] * 4
        L.sqmc_gpu_upload_walkers.argtypes = [C.c_void_p, C.c_int64] + [C.c_void_p] * 9
        L.sqmc_gpu_download_walkers.argtypes = [C.c_void_p, C.c_int64] + [C.c_void_p] * 9
        L.sqmc_gpu_step.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.sqmc_gpu_run.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
        L.sqmc_gpu_det_owner.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
        L.sqmc_gpu_shard_config.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int64, C.c_void_p]
        L.sqmc_gpu_shard_begin.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.sqmc_gpu_shard_pack.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
        L.sqmc_gpu_shard_finish.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
        L.sqmc_gpu_hamiltonian_batch.argtypes = [C.c_void_p, C.c_int64] + [C.c_void_p] * 5
        L.sqmc_gpu_hamiltonian_chem_batch.argtypes = [C.c_void_p, C.c_int64] + [C.c_void_p] * 5
        L.sqmc_gpu_build_sparse_ham.argtypes = [C.c_void_p, C.c_int64] + [C.c_void_p] * 6
        L.sqmc_gpu_propose_batch.argtypes = [C.c_void_p, C.c_int64, C.c_double] + [C.c_void_p] * 7
        L.sqmc_gpu_hci_connections.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_int] + [C.c_void_p] * 5
        L.sqmc_gpu_spmv_prepare.argtypes = [C.c_int64] + [C.c_void_p] * 4
        L.sqmc_gpu_spmv_apply.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
        L.sqmc_gpu_spmv_free.argtypes = [C.c_void_p]
        L.sqmc_gpu_spmv_sym_upper.argtypes = [C.c_int64] + [C.c_void_p] * 5
        L.sqmc_gpu_free.argtypes = [C.c_void_p]
        L.sqmc_gpu_finalize.argtypes = [C.c_void_p]
        L.sqmc_gpu_set_timing.argtypes = [C.c_void_p, C.c_int]
        L.sqmc_gpu_get_timing.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.sqmc_gpu_get_rng.argtypes = [C.c_void_p, C.c_void_p]
        L.sqmc_gpu_set_rng.argtypes = [C.c_void_p, C.c_void_p]
        L.sqmc_gpu_num_walkers.argtypes = [C.c_void_p, C.c_void_p]
        _LIB = L
    return _LIB


def set_device(index):
    L = load_library()
    L.sqmc_gpu_set_device.argtypes = [C.c_int]
    _chk(L.sqmc_gpu_set_device(int(index)))


def _chk(code):
    if code != 0:
        raise SqmcGpuError(code, load_library().sqmc_gpu_last_error().decode())


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _u64(a):
    return np.ascontiguousarray(a, dtype=np.uint64)


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


class GpuChem:
    """One sqmc_gpu_ctx: chemistry tables + (optionally) the walker arrays in HBM."""

    def __init__(self, norb, nup, ndn, orbsym, product_table, combine_2, integrals, n_group=8, time_sym=False, z=1,
                 n_core_orb=0, rng_mode=RNG_COUNTER, seed=(1346, 5634, 6635, 4361), mwalk=0):
        L = load_library()
        self.L = L
        self._tabs = [np.ascontiguousarray(product_table, np.int32), np.ascontiguousarray(orbsym, np.int32),
                      np.ascontiguousarray(combine_2, np.int32), _f64(integrals)]
        cfg = ChemCfg()
        cfg.norb, cfg.nup, cfg.ndn, cfg.n_core_orb = norb, nup, ndn, n_core_orb
        cfg.time_sym, cfg.z, cfg.n_group = int(time_sym), z, n_group
        cfg.product_table, cfg.orbital_symmetries, cfg.combine_2 = (t.ctypes.data for t in self._tabs[:3])
        cfg.n_integrals, cfg.integrals = len(self._tabs[3]) - 1, self._tabs[3].ctypes.data
        cfg.rng_mode, cfg.mwalk = rng_mode, mwalk
        for i in range(4):
            cfg.irand_seed[i] = seed[i]
        h = C.c_void_p()
        _chk(L.sqmc_gpu_init_chem(C.byref(cfg), C.byref(h)))
        self.h, self.norb, self.mwalk = h, norb, mwalk

    @classmethod
    def heg(cls, n_dim, norb, nup, ndn, length_cell, k_vectors, rng_mode=RNG_COUNTER, seed=(1346, 5634, 6635, 4361), mwalk=0):
        """context for the homogeneous electron gas: k_vectors[norb, n_dim] (orbital-major)"""
        self = cls.__new__(cls)
        self.L = L = load_library()
        kv = _f64(np.asarray(k_vectors)[:, :n_dim])
        self._tabs = [kv]
        cfg = HegCfg()
        cfg.n_dim, cfg.norb, cfg.nup, cfg.ndn, cfg.length_cell = n_dim, norb, nup, ndn, float(length_cell)
        cfg.k_vectors, cfg.rng_mode, cfg.mwalk = kv.ctypes.data, rng_mode, mwalk
        for i in range(4):
            cfg.irand_seed[i] = seed[i]
        h = C.c_void_p()
        _chk(L.sqmc_gpu_init_heg(C.byref(cfg), C.byref(h)))
        self.h, self.norb, self.mwalk = h, norb, mwalk
        return self

    @classmethod
    def hubbard(cls, l_x, l_y, pbc, nup, ndn, t, U, rng_mode=RNG_COUNTER, seed=(1346, 5634, 6635, 4361), mwalk=0):
        """context for the real-space Hubbard model on an l_x by l_y lattice ('hubbard2')"""
        self = cls.__new__(cls)
        self.L = L = load_library()
        self._tabs = []
        cfg = HubbardCfg()
        cfg.l_x, cfg.l_y, cfg.pbc, cfg.nup, cfg.ndn, cfg.t, cfg.U = l_x, l_y, int(bool(pbc)), nup, ndn, float(t), float(U)
        cfg.rng_mode, cfg.mwalk = rng_mode, mwalk
        for i in range(4):
            cfg.irand_seed[i] = seed[i]
        h = C.c_void_p()
        _chk(L.sqmc_gpu_init_hubbard(C.byref(cfg), C.byref(h)))
        self.h, self.norb, self.mwalk = h, l_x * l_y, mwalk
        return self

    @classmethod
    def hubbardk(cls, l_x, l_y, nup, ndn, t, U, k_vectors, k_energies, rng_mode=RNG_COUNTER, seed=(1346, 5634, 6635, 4361), mwalk=0):
        """context for the Hubbard model in plane waves ('hubbardk'): k_vectors[nsites, 2] in units of pi / L and k_energies[nsites],
        both in the reference's orbital order (HubbardKHost builds them)"""
        self = cls.__new__(cls)
        self.L = L = load_library()
        kv, ke = np.ascontiguousarray(k_vectors, np.int32).reshape(-1), _f64(k_energies)
        if len(kv) != 2 * l_x * l_y or len(ke) != l_x * l_y:
            raise ValueError("k_vectors / k_energies do not hold l_x * l_y orbitals")
        self._tabs = [kv, ke]
        cfg = HubbardKCfg()
        cfg.l_x, cfg.l_y, cfg.nup, cfg.ndn, cfg.t, cfg.U = l_x, l_y, nup, ndn, float(t), float(U)
        cfg.k_vectors, cfg.k_energies, cfg.rng_mode, cfg.mwalk = kv.ctypes.data, ke.ctypes.data, rng_mode, mwalk
        for i in range(4):
            cfg.irand_seed[i] = seed[i]
        h = C.c_void_p()
        _chk(L.sqmc_gpu_init_hubbardk(C.byref(cfg), C.byref(h)))
        self.h, self.norb, self.mwalk = h, l_x * l_y, mwalk
        return self

    def set_hubbardk_space_sym(self, z, p, c4_map, reflection_map):
        """space_sym = .true. on a hubbardk context: c4_map[nsites, 3] (the reference's c4_map(3, nsites) in memory) and reflection_map[nsites],
        1-based orbital -> 1-based orbital; before walkers, projector and C(T) table"""
        c4, rf = np.ascontiguousarray(c4_map, np.int32), np.ascontiguousarray(reflection_map, np.int32)
        if c4.shape != (self.norb, 3) or rf.shape != (self.norb,):
            raise ValueError("c4_map must be [nsites, 3] and reflection_map [nsites]")
        self.L.sqmc_gpu_set_hubbardk_space_sym.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
        _chk(self.L.sqmc_gpu_set_hubbardk_space_sym(self.h, int(z), int(p), _p(c4), _p(rf)))

    def hubbardk_sym_images(self, up, dn):
        """per determinant: dict of images_up / images_dn [n, 16] and phases [n, 16] in the reference's order, rep_up, rep_dn, phase_w_rep,
        norm and num_distinct (0 where the determinant has no state in the (z, p) sector)"""
        u, d = _u64(up), _u64(dn)
        n = len(u)
        o = dict(images_up=np.zeros((n, 16), np.uint64), images_dn=np.zeros((n, 16), np.uint64), phases=np.zeros((n, 16), np.int32),
                 rep_up=np.zeros(n, np.uint64), rep_dn=np.zeros(n, np.uint64), phase_w_rep=np.zeros(n, np.int32), norm=np.zeros(n),
                 num_distinct=np.zeros(n, np.int32))
        self.L.sqmc_gpu_hubbardk_sym_images.argtypes = [C.c_void_p, C.c_int64] + [C.c_void_p] * 10
        _chk(self.L.sqmc_gpu_hubbardk_sym_images(self.h, n, _p(u), _p(d), *[_p(o[k]) for k in ("images_up", "images_dn", "phases", "rep_up", "rep_dn",
                                                                                                    "phase_w_rep", "norm", "num_distinct")]))
        return o

    def close(self):
        if self.h:
            self.L.sqmc_gpu_finalize(self.h)
            self.h = None

    def set_hb_tables(self, hb_r, hb_s, hb_absH, pq_ind, pq_count, max_double):
        r, s = np.ascontiguousarray(hb_r, np.int32), np.ascontiguousarray(hb_s, np.int32)
        a, pi, pc = _f64(hb_absH), np.ascontiguousarray(pq_ind, np.int64), np.ascontiguousarray(pq_count, np.int32)
        _chk(self.L.sqmc_gpu_set_hb_tables(self.h, len(r), _p(r), _p(s), _p(a), len(pi) - 1, _p(pi), _p(pc), float(max_double)))

    def set_projector(self, counts, indices, values):
        c, i, v = np.ascontiguousarray(counts, np.int64), np.ascontiguousarray(indices, np.int64), _f64(values)
        _chk(self.L.sqmc_gpu_set_projector(self.h, len(c), len(v), _p(c), _p(i), _p(v)))

    def scale_projector(self, ratio):
        _chk(self.L.sqmc_gpu_scale_projector(self.h, float(ratio)))

    def set_ct_table(self, up, dn, num, den):
        u, d, n_, e = _u64(up), _u64(dn), _f64(num), _f64(den)
        _chk(self.L.sqmc_gpu_set_ct_table(self.h, len(u), _p(u), _p(d), _p(n_), _p(e)))

    def set_hf_to_psit(self, psit_ct_index, cdet_psi_t, diag_elems, sum_order=1):
        """hf_to_psit = .true.: after set_projector (matrix without its first row and column) and set_ct_table, before upload_walkers.
        psit_ct_index: 1-based positions of Psi_T's determinants (label order) in the C(T) list."""
        ix, cd, de = np.ascontiguousarray(psit_ct_index, np.int64), _f64(cdet_psi_t), _f64(diag_elems)
        self.L.sqmc_gpu_set_hf_to_psit.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32]
        _chk(self.L.sqmc_gpu_set_hf_to_psit(self.h, len(ix), _p(ix), _p(cd), _p(de), int(sum_order)))

    def upload_walkers(self, w):
        arrs = [_u64(w["up"]), _u64(w["dn"]), _f64(w["wt"]), np.ascontiguousarray(w["imp_distance"], np.int8),
                np.ascontiguousarray(w["initiator"], np.int8), np.ascontiguousarray(w["perm_sign"], np.int8),
                _f64(w["matrix_elements"]), _f64(w["e_num"]), _f64(w["e_den"])]
        _chk(self.L.sqmc_gpu_upload_walkers(self.h, len(arrs[0]), *[_p(a) for a in arrs]))

    def num_walkers(self):
        n = C.c_int64()
        _chk(self.L.sqmc_gpu_num_walkers(self.h, C.byref(n)))
        return n.value

    def download_walkers(self):
        n = self.num_walkers()
        out = dict(up=np.zeros(n, np.uint64), dn=np.zeros(n, np.uint64), wt=np.zeros(n), imp_distance=np.zeros(n, np.int8),
                   initiator=np.zeros(n, np.int8), matrix_elements=np.zeros(n), e_num=np.zeros(n), e_den=np.zeros(n))
        nn = C.c_int64()
        _chk(self.L.sqmc_gpu_download_walkers(self.h, n, C.byref(nn), *[_p(out[k]) for k in
                                              ("up", "dn", "wt", "imp_distance", "initiator", "matrix_elements", "e_num", "e_den")]))
        return out

    def step(self, params):
        p = StepParams(**params)
        out = np.zeros(16)
        code = self.L.sqmc_gpu_step(self.h, C.byref(p), _p(out))
        _chk(code)
        return out

    def annihilate(self, params, spawns):
        """sqmc_gpu_annihilate: caller-supplied spawns (dict up/dn/wt/imp_distance/initiator) through
        sort, merge, rounding and the estimator sums"""
        p = StepParams(**params); out = np.zeros(16)
        arrs = [_u64(spawns["up"]), _u64(spawns["dn"]), _f64(spawns["wt"]), np.ascontiguousarray(spawns["imp_distance"], np.int8),
                np.ascontiguousarray(spawns["initiator"], np.int8)]
        self.L.sqmc_gpu_annihilate.argtypes = [C.c_void_p, C.c_void_p, C.c_int64] + [C.c_void_p] * 6
        _chk(self.L.sqmc_gpu_annihilate(self.h, C.byref(p), len(arrs[0]), *[_p(a) for a in arrs], _p(out)))
        return out

    def debug_premerge(self):
        """sqmc_gpu_debug_premerge (debugging aid, not part of the ABI in include/): the list the last semistochastic radix-tail step or
        sqmc_gpu_annihilate call stood on in front of its merge, as dict(res_wt: the residents' weights after death/clone and the
        projection; up, dn, wt, imp_distance, initiator: the spawn records in creation order, weight 0 meaning no walker).
        The spawn records are valid behind any tail, the last step of a pipelined run() included; res_wt behind the radix tail only."""
        f = self.L.sqmc_gpu_debug_premerge
        f.argtypes = [C.c_void_p, C.c_int64] + [C.c_void_p] * 8
        n0, ns = C.c_int64(), C.c_int64()
        _chk(f(self.h, 0, C.byref(n0), C.byref(ns), None, None, None, None, None, None))
        n0, ns = n0.value, ns.value
        out = dict(res_wt=np.zeros(n0), up=np.zeros(ns, np.uint64), dn=np.zeros(ns, np.uint64), wt=np.zeros(ns), imp_distance=np.zeros(ns, np.int8),
                   initiator=np.zeros(ns, np.int8))
        a, b = C.c_int64(), C.c_int64()
        _chk(f(self.h, n0 + ns, C.byref(a), C.byref(b), *[_p(out[k]) for k in ("res_wt", "up", "dn", "wt", "imp_distance", "initiator")]))
        return out

    def run(self, pc, nsteps, keep_stats=True):
        """sqmc_gpu_run: nsteps steps with the population control done inside the library."""
        stats = np.zeros((nsteps, 16)) if keep_stats else None
        totals = np.zeros(16)
        _chk(self.L.sqmc_gpu_run(self.h, C.byref(pc), int(nsteps), _p(stats) if keep_stats else None, _p(totals)))
        return stats, totals

    # ---- multi-rank sharding (device pointers come from the caller's collective library)
    def det_owner(self, up, dn, nranks):
        u, d = _u64(up), _u64(dn)
        out = np.zeros(len(u), np.int32)
        _chk(self.L.sqmc_gpu_det_owner(self.h, len(u), _p(u), _p(d), int(nranks), _p(out)))
        return out

    def shard_config(self, rank, nranks, global_rows):
        gr = np.ascontiguousarray(global_rows, np.int32)
        _chk(self.L.sqmc_gpu_shard_config(self.h, int(rank), int(nranks), len(gr), _p(gr) if len(gr) else None))

    def shard_begin(self, params, x_global_ptr):
        p = StepParams(**params); n = C.c_int64()
        _chk(self.L.sqmc_gpu_shard_begin(self.h, C.byref(p), C.c_void_p(x_global_ptr), C.byref(n)))
        return n.value

    def shard_pack(self, params, x_global_ptr, send_ptr, cap_records, nranks):
        p = StepParams(**params); cnt = np.zeros(nranks, np.int64)
        _chk(self.L.sqmc_gpu_shard_pack(self.h, C.byref(p), C.c_void_p(x_global_ptr), C.c_void_p(send_ptr), int(cap_records), _p(cnt)))
        return cnt

    def shard_finish(self, params, recv_ptr, n_recv):
        p = StepParams(**params); out = np.zeros(16)
        _chk(self.L.sqmc_gpu_shard_finish(self.h, C.byref(p), C.c_void_p(recv_ptr), int(n_recv), _p(out)))
        return out

    def set_hf_to_psit_shard(self, ct_index, diag_elems, psit_slot, psit_mask, cdet_psi_t, sum_order=1):
        """hf_to_psit on a sharded walk: after shard_config, set_projector and set_ct_table (both global), before upload_walkers.
        ct_index: 1-based positions of this rank's C(T) share in the C(T) list; psit_slot: 1-based slots of its Psi_T entries in that
        share; psit_mask: their 1-based indices in Psi_T (label order); cdet_psi_t: all of Psi_T (psit_shard_tables in host.py)."""
        ix, de = np.ascontiguousarray(ct_index, np.int64), _f64(diag_elems)
        sl, mk, cd = np.ascontiguousarray(psit_slot, np.int64), np.ascontiguousarray(psit_mask, np.int64), _f64(cdet_psi_t)
        self.L.sqmc_gpu_set_hf_to_psit_shard.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                                         C.c_int64, C.c_void_p, C.c_int32]
        _chk(self.L.sqmc_gpu_set_hf_to_psit_shard(self.h, len(ix), _p(ix) if len(ix) else None, _p(de) if len(de) else None, len(sl),
                                                  _p(sl) if len(sl) else None, _p(mk) if len(mk) else None, len(cd), _p(cd), int(sum_order)))

    def shard_finish_psit(self, params, recv_ptr, n_recv, buf_ptr, allreduce):
        """shard_finish of a sharded hf_to_psit step without a communicator: allreduce() is called once, mid-way, after the library has
        written the T^-1 partials (nranks + 1 doubles) to the device buffer at buf_ptr; it must leave their sum over ranks there."""
        p = StepParams(**params); out = np.zeros(16)
        err = []

        def cb(buf, n, user):
            try:
                allreduce()
                return 0
            except Exception as e:          # reported after the library has returned
                err.append(e)
                return 1
        fn = _ALLREDUCE_FN(cb)
        self.L.sqmc_gpu_shard_finish_psit.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, _ALLREDUCE_FN, C.c_void_p, C.c_void_p]
        code = self.L.sqmc_gpu_shard_finish_psit(self.h, C.byref(p), C.c_void_p(recv_ptr), int(n_recv), C.c_void_p(buf_ptr), fn, None, _p(out))
        if err:
            raise err[0]
        _chk(code)
        return out

    # ---- the same with the exchanges inside the library (RCCL)
    @staticmethod
    def comm_unique_id():
        L = load_library(); buf = (C.c_uint8 * 128)()
        L.sqmc_gpu_comm_unique_id.argtypes = [C.c_void_p]
        _chk(L.sqmc_gpu_comm_unique_id(buf))
        return bytes(buf)

    def comm_init(self, unique_id):
        buf = (C.c_uint8 * 128).from_buffer_copy(bytes(unique_id))
        self.L.sqmc_gpu_comm_init.argtypes = [C.c_void_p, C.c_void_p]
        _chk(self.L.sqmc_gpu_comm_init(self.h, buf))

    def shard_time_split(self, reset=False):
        """host wall clock of the in-library sharded steps since the last reset: ({head, exchange, tail, waiting_for_gpu} in us per step, steps)"""
        us, n = (C.c_double * 4)(), C.c_int64()
        self.L.sqmc_gpu_shard_time_split.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32]
        _chk(self.L.sqmc_gpu_shard_time_split(self.h, us, C.byref(n), 1 if reset else 0))
        k = max(n.value, 1)
        return {"head_us": us[0] / k, "exchange_us": us[1] / k, "tail_us": us[2] / k, "of_which_waiting_for_the_gpu_us": us[3] / k}, n.value

    def tail_stats(self):
        """(steps that took the short-list bucket tail, how many of them were re-run through the radix tail)"""
        a, b = C.c_int64(), C.c_int64()
        self.L.sqmc_gpu_tail_stats.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        _chk(self.L.sqmc_gpu_tail_stats(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def last_tail(self):
        """sqmc_gpu_last_tail: the tail the last step took, as dict(kind='radix' | 'bucket' | 'bucket-retried', items=slots per thread
        of the annihilation kernel (0: the bucket kernel), merge=spawn-only sort + merge path taken, packed=keys packed with the indices)"""
        info = (C.c_int32 * 4)()
        self.L.sqmc_gpu_last_tail.argtypes = [C.c_void_p, C.c_void_p]
        _chk(self.L.sqmc_gpu_last_tail(self.h, info))
        return dict(kind=("radix", "bucket", "bucket-retried")[info[0]], items=int(info[1]), merge=bool(info[2]), packed=bool(info[3]))

    def debug_last_head(self):
        """sqmc_gpu_debug_last_head (debugging aid, not part of the ABI in include/): the head the last step() ran behind, as
        dict(pipelined, offsets=who wrote the child offsets, parent_hint, fuse=k_spawn's FUSE form, spare_blocks, proposal)"""
        info = (C.c_int32 * 6)()
        self.L.sqmc_gpu_debug_last_head.argtypes = [C.c_void_p, C.c_void_p]
        _chk(self.L.sqmc_gpu_debug_last_head(self.h, info))
        return dict(pipelined=bool(info[0]), offsets=("gate_scan", "fused_gate_scan", "anneal_lookback", "anneal_bucket", "anneal_split_place", "replay_prepass")[info[1]],
                    parent_hint=bool(info[2]), fuse=bool(info[3]), spare_blocks=int(info[4]), proposal=("uniform", "heatbath", "cauchy", "cauchy_ts")[info[5]])

    def set_chained_runs(self, on):
        """sqmc_gpu_set_chained_runs: keep the step pipeline primed across run() calls (block-structured hosts)"""
        self.L.sqmc_gpu_set_chained_runs.argtypes = [C.c_void_p, C.c_int32]
        _chk(self.L.sqmc_gpu_set_chained_runs(self.h, 1 if on else 0))

    def slowest_steps(self):
        """[(microseconds, step index)] of the four slowest steps of the last run() call"""
        us, st = (C.c_double * 4)(), (C.c_int64 * 4)()
        self.L.sqmc_gpu_slowest_steps.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        _chk(self.L.sqmc_gpu_slowest_steps(self.h, us, st))
        return [(round(us[k], 1), int(st[k])) for k in range(4)]

    def set_owner_hash(self, mode):
        """0: mix of the sort key (default); 1: the reference's djb_hash (mpi_routines.f90:354-379)"""
        self.L.sqmc_gpu_set_owner_hash.argtypes = [C.c_void_p, C.c_int32]
        _chk(self.L.sqmc_gpu_set_owner_hash(self.h, int(mode)))

    def comm_size(self):
        n = C.c_int32()
        self.L.sqmc_gpu_comm_size.argtypes = [C.c_void_p, C.c_void_p]
        _chk(self.L.sqmc_gpu_comm_size(self.h, C.byref(n)))
        return n.value

    def shard_step(self, params):
        p = StepParams(**params); out = np.zeros(16)
        self.L.sqmc_gpu_shard_step.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        _chk(self.L.sqmc_gpu_shard_step(self.h, C.byref(p), _p(out)))
        return out

    def shard_run(self, pc, nsteps, keep_stats=True):
        stats = np.zeros((nsteps, 16)) if keep_stats else None
        totals = np.zeros(16)
        self.L.sqmc_gpu_shard_run.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
        _chk(self.L.sqmc_gpu_shard_run(self.h, C.byref(pc), int(nsteps), _p(stats) if keep_stats else None, _p(totals)))
        return stats, totals

    def rng_state(self):
        s = (C.c_int32 * 4)()
        _chk(self.L.sqmc_gpu_get_rng(self.h, s))
        return list(s)

    def set_rng(self, seed):
        """re-seeds the context from four 12-bit limbs (setrn: the last one made odd), in either RNG discipline"""
        s = (C.c_int32 * 4)(*[int(x) for x in seed])
        _chk(self.L.sqmc_gpu_set_rng(self.h, s))

    def set_timing(self, level=2):
        _chk(self.L.sqmc_gpu_set_timing(self.h, int(level)))

    def timing(self):
        n = C.c_int32(); names = (C.c_char_p * 32)(); ms = (C.c_float * 32)()
        _chk(self.L.sqmc_gpu_get_timing(self.h, C.byref(n), names, ms))
        return [(names[i].decode(), ms[i]) for i in range(n.value)]

    def hamiltonian_batch(self, iu, id_, ju, jd):
        a, b, c, d = _u64(iu), _u64(id_), _u64(ju), _u64(jd)
        h = np.zeros(len(a))
        _chk(self.L.sqmc_gpu_hamiltonian_batch(self.h, len(a), _p(a), _p(b), _p(c), _p(d), _p(h)))
        return h

    def hamiltonian_chem_batch(self, iu, id_, ju, jd):
        a, b, c, d = _u64(iu), _u64(id_), _u64(ju), _u64(jd)
        h = np.zeros(len(a))
        _chk(self.L.sqmc_gpu_hamiltonian_chem_batch(self.h, len(a), _p(a), _p(b), _p(c), _p(d), _p(h)))
        return h

    def build_sparse_ham(self, up, dn):
        u, d = _u64(up), _u64(dn)
        n = len(u)
        nnz = C.c_int64(); prc = C.c_void_p(); pix = C.c_void_p(); pvl = C.c_void_p()
        _chk(self.L.sqmc_gpu_build_sparse_ham(self.h, n, _p(u), _p(d), C.byref(nnz), C.byref(prc), C.byref(pix), C.byref(pvl)))
        k = nnz.value
        rc = np.ctypeslib.as_array(C.cast(prc, C.POINTER(C.c_int64)), shape=(n,)).copy()
        ix = np.ctypeslib.as_array(C.cast(pix, C.POINTER(C.c_int64)), shape=(k,)).copy()
        vl = np.ctypeslib.as_array(C.cast(pvl, C.POINTER(C.c_double)), shape=(k,)).copy()
        for q in (prc, pix, pvl):
            self.L.sqmc_gpu_free(q)
        return rc, ix, vl

    def set_heatbath_tables(self, tabs):
        """tabs: dict with the reference's arrays in the reference's (Fortran, column-major) order -- see sqmc_heatbath_tables"""
        t = HeatbathTables()
        keep = []
        def put(name, arr, dt):
            a = np.ascontiguousarray(arr, dt).reshape(-1); keep.append(a)
            setattr(t, name, a.ctypes.data_as(C.c_void_p))
        t.norb = int(tabs["norb"])
        put("one", tabs["one"], np.float64); put("two", tabs["two"], np.float64)
        put("three_same", tabs["three_same"], np.float64); put("three_opp", tabs["three_opp"], np.float64)
        put("j3_same", tabs["j3_same"], np.int32); put("j3_opp", tabs["j3_opp"], np.int32)
        put("q3_same", tabs["q3_same"], np.float64); put("q3_opp", tabs["q3_opp"], np.float64)
        t.size_same, t.size_opp = int(tabs["size_same"]), int(tabs["size_opp"])
        put("four_same", tabs["four_same"], np.float32); put("four_opp", tabs["four_opp"], np.float32)
        put("j4_same", tabs["j4_same"], np.int32); put("j4_opp", tabs["j4_opp"], np.int32)
        put("q4_same", tabs["q4_same"], np.float32); put("q4_opp", tabs["q4_opp"], np.float32)
        put("htot_same", tabs["htot_same"], np.float64); put("htot_opp", tabs["htot_opp"], np.float64)
        self.L.sqmc_gpu_set_heatbath_tables.argtypes = [C.c_void_p, C.c_void_p]
        _chk(self.L.sqmc_gpu_set_heatbath_tables(self.h, C.byref(t)))

    def setup_efficient_heatbath(self):
        """setup_efficient_heatbath + check_heatbath_unbiased done by the library (proposal_method fast_heatbath from here on if the
        check passes).  Returns is_heatbath_unbiased."""
        ok = C.c_int32()
        self.L.sqmc_gpu_setup_efficient_heatbath.argtypes = [C.c_void_p, C.c_void_p]
        _chk(self.L.sqmc_gpu_setup_efficient_heatbath(self.h, C.byref(ok)))
        return bool(ok.value)

    def heatbath_tables(self):
        """the tables the library built (copies, the reference's layout as in sqmc_heatbath_tables) and the number of orbitals of unique symmetry"""
        t, nu = HeatbathTables(), C.c_int32()
        self.L.sqmc_gpu_get_heatbath_tables.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        _chk(self.L.sqmc_gpu_get_heatbath_tables(self.h, C.byref(t), C.byref(nu)))
        n = t.norb
        npairs = (n * (n - 1)) // 2 + n

        def take(ptr, count, dt):
            return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(dt)), shape=(count,)).copy()
        out = dict(norb=n, size_same=t.size_same, size_opp=t.size_opp, n_orb_uniq_sym=nu.value,
                   one=take(t.one, n, C.c_double), two=take(t.two, 4 * n * n, C.c_double),
                   three_same=take(t.three_same, n ** 3, C.c_double), three_opp=take(t.three_opp, n ** 3, C.c_double),
                   j3_same=take(t.j3_same, n ** 3, C.c_int32), j3_opp=take(t.j3_opp, n ** 3, C.c_int32),
                   q3_same=take(t.q3_same, n ** 3, C.c_double), q3_opp=take(t.q3_opp, n ** 3, C.c_double),
                   four_same=take(t.four_same, t.size_same, C.c_float), four_opp=take(t.four_opp, t.size_opp, C.c_float),
                   j4_same=take(t.j4_same, t.size_same, C.c_int32), j4_opp=take(t.j4_opp, t.size_opp, C.c_int32),
                   q4_same=take(t.q4_same, t.size_same, C.c_float), q4_opp=take(t.q4_opp, t.size_opp, C.c_float),
                   htot_same=take(t.htot_same, npairs * n, C.c_double), htot_opp=take(t.htot_opp, n ** 3, C.c_double))
        return out

    def propose_heatbath_batch(self, tau, up, dn, seeds):
        u, d = _u64(up), _u64(dn)
        s = np.ascontiguousarray(seeds, np.int32).reshape(-1)
        n = len(u)
        ju, jd, wj, sa = np.zeros(2 * n, np.uint64), np.zeros(2 * n, np.uint64), np.zeros(2 * n), np.zeros(4 * n, np.int32)
        self.L.sqmc_gpu_propose_heatbath_batch.argtypes = [C.c_void_p, C.c_int64, C.c_double] + [C.c_void_p] * 7
        _chk(self.L.sqmc_gpu_propose_heatbath_batch(self.h, n, float(tau), _p(u), _p(d), _p(s), _p(ju), _p(jd), _p(wj), _p(sa)))
        return ju.reshape(n, 2), jd.reshape(n, 2), wj.reshape(n, 2), sa.reshape(n, 4)

    def setup_cauchy_schwarz(self):
        """proposal_method CauchySchwarz from here on: setup_orb_by_symm's tables, with its stop on an exchange integral below -1e-6
        (SqmcGpuError "Negative integrals!") and its clamp of the slightly negative ones to 0.  Returns how many were clamped."""
        n = C.c_int32(0)
        self.L.sqmc_gpu_setup_cauchy_schwarz.argtypes = [C.c_void_p, C.c_void_p]
        _chk(self.L.sqmc_gpu_setup_cauchy_schwarz(self.h, C.byref(n)))
        return int(n.value)

    def propose_cauchy_schwarz_batch(self, tau, up, dn, seeds):
        """n Cauchy-Schwarz proposals, proposal i from the rannyu state seeds[i] (4 limbs): det_j, weight_j (0: no move), seeds after"""
        u, d = _u64(up), _u64(dn)
        s = np.ascontiguousarray(seeds, np.int32).reshape(-1)
        n = len(u)
        ju, jd, wj, sa = np.zeros(n, np.uint64), np.zeros(n, np.uint64), np.zeros(n), np.zeros(4 * n, np.int32)
        self.L.sqmc_gpu_propose_cauchy_schwarz_batch.argtypes = [C.c_void_p, C.c_int64, C.c_double] + [C.c_void_p] * 7
        _chk(self.L.sqmc_gpu_propose_cauchy_schwarz_batch(self.h, n, float(tau), _p(u), _p(d), _p(s), _p(ju), _p(jd), _p(wj), _p(sa)))
        return ju, jd, wj, sa.reshape(n, 4)

    def propose_batch(self, tau, up, dn, seeds):
        u, d = _u64(up), _u64(dn)
        s = np.ascontiguousarray(seeds, np.int32).reshape(-1)
        n = len(u)
        ju, jd, wj, sa = np.zeros(n, np.uint64), np.zeros(n, np.uint64), np.zeros(n), np.zeros(4 * n, np.int32)
        _chk(self.L.sqmc_gpu_propose_batch(self.h, n, float(tau), _p(u), _p(d), _p(s), _p(ju), _p(jd), _p(wj), _p(sa)))
        return ju, jd, wj, sa.reshape(n, 4)

    def hci_connections(self, ref_up, ref_dn, coeffs, eps, diag_mode=0, slice=0, n_slices=1):
        u, d, c = _u64(ref_up), _u64(ref_dn), _f64(coeffs)
        n = C.c_int64(); pu = C.c_void_p(); pd = C.c_void_p(); pn = C.c_void_p(); pe = C.c_void_p()
        self.L.sqmc_gpu_hci_connections_slice.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_int,
                                                          C.c_int32, C.c_int32] + [C.c_void_p] * 5
        _chk(self.L.sqmc_gpu_hci_connections_slice(self.h, len(u), _p(u), _p(d), _p(c), float(eps), int(diag_mode), int(slice), int(n_slices),
                                                   C.byref(n), C.byref(pu), C.byref(pd), C.byref(pn), C.byref(pe)))
        k = n.value
        if k == 0:
            return np.zeros(0, np.uint64), np.zeros(0, np.uint64), np.zeros(0), np.zeros(0)
        def take(ptr, ct, dt):
            a = np.ctypeslib.as_array(C.cast(ptr, C.POINTER(ct)), shape=(max(k, 1),))[:k].astype(dt, copy=True)
            self.L.sqmc_gpu_free(ptr)
            return a
        return take(pu, C.c_uint64, np.uint64), take(pd, C.c_uint64, np.uint64), take(pn, C.c_double, np.float64), take(pe, C.c_double, np.float64)


def _gpuchem_hci_set_active_space(self, core_up, core_dn, virt_up, virt_dn, mode):
    """masks of the HCI generator: mode 0 none, 1 inside the active space only, 2 outside only"""
    self.L.sqmc_gpu_hci_set_active_space.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, C.c_int32]
    _chk(self.L.sqmc_gpu_hci_set_active_space(self.h, int(core_up), int(core_dn), int(virt_up), int(virt_dn), int(mode)))


def _gpuchem_diag_update_batch(self, old_diag, pqrs, new_up, new_dn, form=0):
    """sqmc_gpu_diag_update_batch (get_new_diag_elem): H_aa of new_up/new_dn[i] from old_diag[i] = H of its source and pqrs[i] = (p, q, r, s),
    the excitation in the reference's 1..2 norb spin-orbital numbering.  form 0: one lane, reference order; 1: 16-lane groups."""
    o, u, d = _f64(old_diag), _u64(new_up), _u64(new_dn)
    q = np.ascontiguousarray(pqrs, np.int32).reshape(-1)
    n = len(o)
    if len(q) != 4 * n or len(u) != n or len(d) != n:
        raise ValueError("old_diag, pqrs (4 per record), new_up and new_dn differ in length")
    out = np.zeros(n)
    self.L.sqmc_gpu_diag_update_batch.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
    _chk(self.L.sqmc_gpu_diag_update_batch(self.h, n, _p(o), _p(q), _p(u), _p(d), int(form), _p(out)))
    return out


def _gpuchem_hci_set_diag_update(self, mode):
    """H_aa of the PT2 stages: 0 from scratch (default), 1 the O(N) update on one lane, 2 the same by 16-lane groups"""
    self.L.sqmc_gpu_hci_set_diag_update.argtypes = [C.c_void_p, C.c_int32]
    _chk(self.L.sqmc_gpu_hci_set_diag_update(self.h, int(mode)))


def _gpuchem_hci_connections_record(self, ref_up, ref_dn, coeffs, eps, diag_mode=0, slice=0, n_slices=1):
    """hci_connections with the update's record of every connection: (up, dn, num, den, old_diag, pqrs[n, 4])"""
    u, d, c = _u64(ref_up), _u64(ref_dn), _f64(coeffs)
    n = C.c_int64(); ptr = [C.c_void_p() for _ in range(6)]
    self.L.sqmc_gpu_hci_connections_record.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_int,
                                                       C.c_int32, C.c_int32] + [C.c_void_p] * 7
    _chk(self.L.sqmc_gpu_hci_connections_record(self.h, len(u), _p(u), _p(d), _p(c), float(eps), int(diag_mode), int(slice), int(n_slices),
                                                C.byref(n), *[C.byref(x) for x in ptr]))
    k = n.value
    if k == 0:
        return np.zeros(0, np.uint64), np.zeros(0, np.uint64), np.zeros(0), np.zeros(0), np.zeros(0), np.zeros((0, 4), np.int32)
    def take(x, ct, dt, m):
        a = np.ctypeslib.as_array(C.cast(x, C.POINTER(ct)), shape=(m,)).astype(dt, copy=True)
        self.L.sqmc_gpu_free(x)
        return a
    return (take(ptr[0], C.c_uint64, np.uint64, k), take(ptr[1], C.c_uint64, np.uint64, k), take(ptr[2], C.c_double, np.float64, k),
            take(ptr[3], C.c_double, np.float64, k), take(ptr[4], C.c_double, np.float64, k), take(ptr[5], C.c_int32, np.int32, 4 * k).reshape(k, 4))


def _gpuchem_hci_pt2(self, up, dn, coeffs, e_var, eps_pt, n_slices=1):
    """sqmc_gpu_hci_pt2: (delta_E, number of connected determinants), everything on the device"""
    u, d, c = _u64(up), _u64(dn), _f64(coeffs)
    de, nc = C.c_double(), C.c_int64()
    self.L.sqmc_gpu_hci_pt2.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_double, C.c_int32, C.c_void_p, C.c_void_p]
    _chk(self.L.sqmc_gpu_hci_pt2(self.h, len(u), _p(u), _p(d), _p(c), float(e_var), float(eps_pt), int(n_slices), C.byref(de), C.byref(nc)))
    return de.value, nc.value


def _gpuchem_one_rdm(self, up, dn, coeffs, orbital_symmetries=None):
    """sqmc_gpu_hci_1rdm (get_1rdm, hci.f90:3198-3398): the spin-traced one-body density matrix of a determinant list in any order as
    an (norb, norb) array, a[p, r] = sum_sigma <psi| a+_r a_p |psi> (the electron moves p -> r; 0-based).  orbital_symmetries: norb
    labels, pairs of different label are skipped and exactly 0.0"""
    u, d, c = _u64(up), _u64(dn), _f64(coeffs)
    if not (len(u) == len(d) == len(c)):
        raise ValueError("up, dn and coeffs differ in length")
    sym = None if orbital_symmetries is None else np.ascontiguousarray(orbital_symmetries, np.int32)
    if sym is not None and len(sym) != self.norb:
        raise ValueError("orbital_symmetries must hold norb labels")
    out = np.zeros(self.norb * self.norb)
    self.L.sqmc_gpu_hci_1rdm.argtypes = [C.c_void_p, C.c_int64] + [C.c_void_p] * 5
    _chk(self.L.sqmc_gpu_hci_1rdm(self.h, len(u), _p(u), _p(d), _p(c), None if sym is None else _p(sym), _p(out)))
    return np.ascontiguousarray(out.reshape(self.norb, self.norb).T)          # flat index p + norb r


def _gpuchem_one_rdm_pt(self, up, dn, coeffs, e_var, eps_pt_big, n_slices=1):
    """sqmc_gpu_hci_1rdm_pt (get_1rdm_with_pt, hci.f90:3400-3551): (<0|rho|0> + <0|rho|1> + <1|rho|0> as an (norb, norb) array indexed
    as one_rdm's, connected determinants visited)"""
    u, d, c = _u64(up), _u64(dn), _f64(coeffs)
    if not (len(u) == len(d) == len(c)):
        raise ValueError("up, dn and coeffs differ in length")
    out, nc = np.zeros(self.norb * self.norb), C.c_int64()
    self.L.sqmc_gpu_hci_1rdm_pt.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_double, C.c_int32, C.c_void_p, C.c_void_p]
    _chk(self.L.sqmc_gpu_hci_1rdm_pt(self.h, len(u), _p(u), _p(d), _p(c), float(e_var), float(eps_pt_big), int(n_slices), _p(out), C.byref(nc)))
    return np.ascontiguousarray(out.reshape(self.norb, self.norb).T), nc.value


_RDM2_BLOCKS = {"aa": 1, "bb": 2, "ab": 4}


def _gpuchem_two_rdm(self, up, dn, coeffs, blocks="all"):
    """sqmc_gpu_hci_2rdm: the spin blocks of the two-body density matrix of a determinant list in any order, a dict of (norb,) * 4
    arrays in Fortran order keyed "aa", "bb", "ab": G_aa[p, q, r, s] = <a+_{p up} a+_{q up} a_{s up} a_{r up}>, G_bb the same with dn,
    G_ab[p, q, r, s] = <a+_{p up} a+_{q dn} a_{s dn} a_{r up}> (0-based; nothing is renormalised).  blocks: "all", one of the keys, or a
    sequence of them; only those are computed and returned"""
    u, d, c = _u64(up), _u64(dn), _f64(coeffs)
    if not (len(u) == len(d) == len(c)):
        raise ValueError("up, dn and coeffs differ in length")
    names = ("aa", "bb", "ab") if blocks == "all" else (blocks,) if isinstance(blocks, str) else tuple(blocks)
    if not names or any(b not in _RDM2_BLOCKS for b in names):
        raise ValueError("two_rdm: blocks must be 'all' or among 'aa', 'bb', 'ab'")
    out = {b: np.zeros(self.norb ** 4) for b in ("aa", "bb", "ab") if b in names}
    self.L.sqmc_gpu_hci_2rdm.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    _chk(self.L.sqmc_gpu_hci_2rdm(self.h, len(u), _p(u), _p(d), _p(c), sum(_RDM2_BLOCKS[b] for b in out),
                                  *[_p(out[b]) if b in out else None for b in ("aa", "bb", "ab")]))
    return {b: a.reshape((self.norb,) * 4, order="F") for b, a in out.items()}


def _gpuchem_rotate_integrals(self, rot):
    """sqmc_gpu_rotate_integrals (the rotation of generate_natorb_integrals, hci.f90:3683-3791): the context's integrals in the orbitals
    new_p = sum_k rot[k, p] old_k, as a new packed array of n_integrals + 1 doubles addressed by the same combine_2.  rot: (norb, norb),
    the `vectors` of host.natural_orbitals; any finite real matrix."""
    u = _f64(rot)
    if u.shape != (self.norb, self.norb):
        raise ValueError("rotate_integrals: rot must be (norb, norb) = (%d, %d), got %r" % (self.norb, self.norb, u.shape))
    out = np.zeros(len(self._tabs[3]) if len(self._tabs) > 3 else 1)      # (the library refuses a context without an integral table)
    self.L.sqmc_gpu_rotate_integrals.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    _chk(self.L.sqmc_gpu_rotate_integrals(self.h, _p(u), _p(out)))
    return out


def _gpuchem_one_tdm(self, up, dn, bra, ket, orbital_symmetries=None):
    """sqmc_gpu_hci_1tdm: the spin-summed one-body transition density matrix of two coefficient vectors over one determinant list in
    any order as an (norb, norb) array indexed as one_rdm's, a[p, r] = <bra| a+_r a_p |ket> (the electron moves p -> r; 0-based;
    nothing is renormalised).  one_tdm(bra, ket) == one_tdm(ket, bra).T exactly.  orbital_symmetries: as in one_rdm"""
    u, d, b, k = _u64(up), _u64(dn), _f64(bra), _f64(ket)
    if not (len(u) == len(d) == len(b) == len(k)):
        raise ValueError("up, dn, bra and ket differ in length")
    sym = None if orbital_symmetries is None else np.ascontiguousarray(orbital_symmetries, np.int32)
    if sym is not None and len(sym) != self.norb:
        raise ValueError("orbital_symmetries must hold norb labels")
    out = np.zeros(self.norb * self.norb)
    self.L.sqmc_gpu_hci_1tdm.argtypes = [C.c_void_p, C.c_int64] + [C.c_void_p] * 6
    _chk(self.L.sqmc_gpu_hci_1tdm(self.h, len(u), _p(u), _p(d), _p(b), _p(k), None if sym is None else _p(sym), _p(out)))
    return np.ascontiguousarray(out.reshape(self.norb, self.norb).T)          # flat index p + norb r


def _gpuchem_two_tdm(self, up, dn, bra, ket, blocks="all"):
    """sqmc_gpu_hci_2tdm: the spin blocks of the two-body transition density matrix of two coefficient vectors over one determinant
    list in any order, a dict as two_rdm's: T_aa[p, q, r, s] = <bra| a+_{p up} a+_{q up} a_{s up} a_{r up} |ket>, T_bb the same with
    dn, T_ab[p, q, r, s] = <bra| a+_{p up} a+_{q dn} a_{s dn} a_{r up} |ket> (0-based; nothing is renormalised).
    two_tdm(bra, ket)[b] == two_tdm(ket, bra)[b].transpose(2, 3, 0, 1) and two_tdm(c, c) == two_rdm(c), both exactly"""
    u, d, b, k = _u64(up), _u64(dn), _f64(bra), _f64(ket)
    if not (len(u) == len(d) == len(b) == len(k)):
        raise ValueError("up, dn, bra and ket differ in length")
    names = ("aa", "bb", "ab") if blocks == "all" else (blocks,) if isinstance(blocks, str) else tuple(blocks)
    if not names or any(x not in _RDM2_BLOCKS for x in names):
        raise ValueError("two_tdm: blocks must be 'all' or among 'aa', 'bb', 'ab'")
    out = {x: np.zeros(self.norb ** 4) for x in ("aa", "bb", "ab") if x in names}
    self.L.sqmc_gpu_hci_2tdm.argtypes = [C.c_void_p, C.c_int64] + [C.c_void_p] * 4 + [C.c_int32] + [C.c_void_p] * 3
    _chk(self.L.sqmc_gpu_hci_2tdm(self.h, len(u), _p(u), _p(d), _p(b), _p(k), sum(_RDM2_BLOCKS[x] for x in out),
                                  *[_p(out[x]) if x in out else None for x in ("aa", "bb", "ab")]))
    return {x: a.reshape((self.norb,) * 4, order="F") for x, a in out.items()}


_ORBOPT_OUT = ("fock", "gradient", "hdiag")


def _gpuchem_orbital_gradient(self, one_rdm, two_rdm_sf, outputs="all"):
    """sqmc_gpu_orbital_gradient: the generalised Fock matrix, the orbital gradient and the diagonal orbital Hessian of the
    fixed-coefficient energy from the spin-summed one-body matrix (one_rdm's [p, r]) and the spin-free two-body matrix
    (host.spin_free_two_rdm's [p, q, r, s]) on the context's integrals: a dict of (norb, norb) arrays "fock" [a, P], "gradient" and
    "hdiag" [p, q] (0-based; dE/dtheta and d2E/dtheta2 at 0 along exp(theta (e_p e_q^T - e_q e_p^T)), rotations as rotate_integrals').
    outputs: "all", one of the keys, or a sequence of them; only those are computed and returned"""
    n = self.norb
    d = np.asarray(one_rdm, np.float64)
    gg = np.asarray(two_rdm_sf, np.float64)
    if d.shape != (n, n) or gg.shape != (n,) * 4:
        raise ValueError("orbital_gradient: one_rdm must be (norb, norb) and two_rdm_sf (norb,) * 4 with norb = %d, got %r and %r" % (n, d.shape, gg.shape))
    names = _ORBOPT_OUT if outputs == "all" else (outputs,) if isinstance(outputs, str) else tuple(outputs)
    if not names or any(b not in _ORBOPT_OUT for b in names):
        raise ValueError("orbital_gradient: outputs must be 'all' or among 'fock', 'gradient', 'hdiag'")
    d, gg = np.ascontiguousarray(d.reshape(-1, order="F")), np.ascontiguousarray(gg.reshape(-1, order="F"))
    out = {b: np.zeros(n * n) for b in _ORBOPT_OUT if b in names}
    self.L.sqmc_gpu_orbital_gradient.argtypes = [C.c_void_p] * 6
    _chk(self.L.sqmc_gpu_orbital_gradient(self.h, _p(d), _p(gg), *[_p(out[b]) if b in out else None for b in _ORBOPT_OUT]))
    return {b: a.reshape((n, n), order="F") for b, a in out.items()}


def _gpuchem_one_index_transform(self, kappa):
    """sqmc_gpu_one_index_transform: the first-order coefficient in t of rotate_integrals(I + t kappa) as a packed array of
    n_integrals + 1 doubles addressed by the same combine_2 (the nuclear-energy slot is 0.0).  kappa: (norb, norb), [a, P] as rot;
    any finite real matrix."""
    k = _f64(kappa)
    if k.shape != (self.norb, self.norb):
        raise ValueError("one_index_transform: kappa must be (norb, norb) = (%d, %d), got %r" % (self.norb, self.norb, k.shape))
    out = np.zeros(len(self._tabs[3]) if len(self._tabs) > 3 else 1)      # (the library refuses a context without an integral table)
    self.L.sqmc_gpu_one_index_transform.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    _chk(self.L.sqmc_gpu_one_index_transform(self.h, _p(k), _p(out)))
    return out


class OrbOptPlan:
    """sqmc_gpu_orbopt_prepare / _gradient / _hessian_vector / _free: the density matrices of GpuChem.orbital_gradient resident on the
    device, F, gradient and hdiag computed once, and the orbital Hessian of the fixed-coefficient energy applied to antisymmetric
    matrices.  The plan borrows the context g: close it before g."""

    def __init__(self, g, one_rdm, two_rdm_sf):
        self.L, self.norb, self.h = g.L, g.norb, None
        n = g.norb
        d = np.asarray(one_rdm, np.float64)
        gg = np.asarray(two_rdm_sf, np.float64)
        if d.shape != (n, n) or gg.shape != (n,) * 4:
            raise ValueError("orbopt_plan: one_rdm must be (norb, norb) and two_rdm_sf (norb,) * 4 with norb = %d, got %r and %r" % (n, d.shape, gg.shape))
        d, gg = np.ascontiguousarray(d.reshape(-1, order="F")), np.ascontiguousarray(gg.reshape(-1, order="F"))
        self.L.sqmc_gpu_orbopt_prepare.argtypes = [C.c_void_p] * 4
        self.L.sqmc_gpu_orbopt_gradient.argtypes = [C.c_void_p] * 4
        self.L.sqmc_gpu_orbopt_hessian_vector.argtypes = [C.c_void_p] * 3
        self.L.sqmc_gpu_orbopt_free.argtypes = [C.c_void_p]
        h = C.c_void_p()
        _chk(self.L.sqmc_gpu_orbopt_prepare(g.h, _p(d), _p(gg), C.byref(h)))
        self.h, self.g = h, g

    def gradient(self, outputs="all"):
        """GpuChem.orbital_gradient's dict on the plan's matrices, the same bits, without another upload or kernel"""
        n = self.norb
        names = _ORBOPT_OUT if outputs == "all" else (outputs,) if isinstance(outputs, str) else tuple(outputs)
        if not names or any(b not in _ORBOPT_OUT for b in names):
            raise ValueError("OrbOptPlan.gradient: outputs must be 'all' or among 'fock', 'gradient', 'hdiag'")
        out = {b: np.zeros(n * n) for b in _ORBOPT_OUT if b in names}
        _chk(self.L.sqmc_gpu_orbopt_gradient(self.h, *[_p(out[b]) if b in out else None for b in _ORBOPT_OUT]))
        return {b: a.reshape((n, n), order="F") for b, a in out.items()}

    def hessian_vector(self, kappa):
        """sigma[p, q] = d2 E(exp(s kappa + t K_pq)) / ds dt at 0 for an exactly antisymmetric (norb, norb) kappa"""
        n = self.norb
        k = _f64(kappa)
        if k.shape != (n, n):
            raise ValueError("OrbOptPlan.hessian_vector: kappa must be (norb, norb) = (%d, %d), got %r" % (n, n, k.shape))
        out = np.zeros(n * n)
        _chk(self.L.sqmc_gpu_orbopt_hessian_vector(self.h, _p(k), _p(out)))
        return out.reshape((n, n), order="F")

    def close(self):
        if self.h:
            self.L.sqmc_gpu_orbopt_free(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def _gpuchem_orbopt_plan(self, one_rdm, two_rdm_sf):
    """an OrbOptPlan on this context's integrals (close it before the context)"""
    return OrbOptPlan(self, one_rdm, two_rdm_sf)


def _gpuchem_greens_function(self, up, dn, coeffs, e0, w, fermi_sign=False, parts="both"):
    """sqmc_gpu_hci_greens_function (get_zeroth_order_variational_greens_function, hci.f90:3849-4050): (G_np1, G_nm1) of a determinant
    list in any order at the frequencies w, each an (n_w, norb, norb) array indexed [i_w, p, q] (0-based), spin-summed.  fermi_sign
    False: no fermionic sign, as the reference; True: the matrix elements of a_p .. a+_q and a+_p .. a_q.  parts: "both", "np1" or
    "nm1"; the half that is not asked for is not computed and comes back as None."""
    u, d, c, ww = _u64(up), _u64(dn), _f64(coeffs), np.ascontiguousarray(np.atleast_1d(w), np.float64)
    if not (len(u) == len(d) == len(c)):
        raise ValueError("up, dn and coeffs differ in length")
    if parts not in ("both", "np1", "nm1"):
        raise ValueError("parts must be 'both', 'np1' or 'nm1'")
    n = self.norb
    gp = np.zeros(len(ww) * n * n) if parts != "nm1" else None
    gm = np.zeros(len(ww) * n * n) if parts != "np1" else None
    self.L.sqmc_gpu_hci_greens_function.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_int32, C.c_void_p, C.c_int32,
                                                    C.c_void_p, C.c_void_p]
    _chk(self.L.sqmc_gpu_hci_greens_function(self.h, len(u), _p(u), _p(d), _p(c), float(e0), len(ww), _p(ww), int(fermi_sign),
                                             None if gp is None else _p(gp), None if gm is None else _p(gm)))
    shape = lambda a: None if a is None else np.ascontiguousarray(a.reshape(n, n, len(ww)).transpose(2, 1, 0))      # flat index i_w + n_w (p + norb q)
    return shape(gp), shape(gm)


class HeatbathTables(C.Structure):
    """sqmc_heatbath_tables of include/sqmc_gpu.h"""
    _fields_ = [("norb", C.c_int32), ("reserved", C.c_int32), ("one", C.c_void_p), ("two", C.c_void_p), ("three_same", C.c_void_p), ("three_opp", C.c_void_p),
                ("j3_same", C.c_void_p), ("j3_opp", C.c_void_p), ("q3_same", C.c_void_p), ("q3_opp", C.c_void_p), ("size_same", C.c_int64), ("size_opp", C.c_int64),
                ("four_same", C.c_void_p), ("four_opp", C.c_void_p), ("j4_same", C.c_void_p), ("j4_opp", C.c_void_p), ("q4_same", C.c_void_p), ("q4_opp", C.c_void_p),
                ("htot_same", C.c_void_p), ("htot_opp", C.c_void_p)]


class SpmvPlan:
    """sqmc_gpu_spmv_prepare/apply: symmetric matvec of davidson_sparse (more_tools.f90:2115)."""

    def __init__(self, counts, indices, values):
        self.L = load_library()
        c, i, v = np.ascontiguousarray(counts, np.int64), np.ascontiguousarray(indices, np.int64), _f64(values)
        self.n = len(c)
        h = C.c_void_p()
        _chk(self.L.sqmc_gpu_spmv_prepare(self.n, _p(c), _p(i), _p(v), C.byref(h)))
        self.h = h

    @classmethod
    def from_dets(cls, g, up, dn):
        """sqmc_gpu_build_spmv_plan: Hamiltonian of a sorted determinant list built and kept on the GPU.
        Returns (plan, diagonal, stored upper-triangular nonzeros)."""
        self = cls.__new__(cls)
        self.L = g.L
        u, d = _u64(up), _u64(dn)
        self.n = len(u)
        diag = np.zeros(self.n); nnz = C.c_int64(); h = C.c_void_p()
        self.L.sqmc_gpu_build_spmv_plan.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        _chk(self.L.sqmc_gpu_build_spmv_plan(g.h, self.n, _p(u), _p(d), C.byref(h), _p(diag), C.byref(nnz)))
        self.h = h
        return self, diag, nnz.value

    def submatrix(self, sel):
        """sqmc_gpu_spmv_plan_submatrix: the plan of the principal submatrix on the rows sel (0-based, strictly ascending), extracted on the
        device from this plan, which stays as it is.  Entry for entry the plan built from the subset itself; its preconditioner is
        diag[sel].  nnz_full of the result: the entries of its full CSR."""
        s = np.ascontiguousarray(sel, np.int64) + 1
        new = type(self).__new__(type(self))
        new.L, new.n, new.h = self.L, len(s), None
        h = C.c_void_p(); nnz = C.c_int64()
        self.L.sqmc_gpu_spmv_plan_submatrix.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]
        _chk(self.L.sqmc_gpu_spmv_plan_submatrix(self.h, len(s), _p(s) if len(s) else None, C.byref(h), C.byref(nnz)))
        new.h, new.nnz_full = h, nnz.value
        return new

    def apply(self, x):
        x = _f64(x); y = np.zeros(self.n)
        _chk(self.L.sqmc_gpu_spmv_apply(self.h, _p(x), _p(y), 0))
        return y

    def davidson(self, diag, k=1, v0=None, tol=1e-10):
        """sqmc_gpu_davidson: lowest k eigenpairs, basis and products resident on the device.  Returns (eigenvalues[k], vectors[n, k], matvecs)"""
        d = _f64(diag)
        ev = np.zeros(k); X = np.zeros((k, self.n)); nm = C.c_int32()
        s = None if v0 is None else np.ascontiguousarray(np.asarray(v0, float).reshape(self.n, -1)[:, :k].T)       # column-major n x k
        self.L.sqmc_gpu_davidson.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p]
        _chk(self.L.sqmc_gpu_davidson(self.h, _p(d), int(k), None if s is None else _p(s), float(tol), _p(ev), _p(X), C.byref(nm)))
        return ev, np.ascontiguousarray(X.T), nm.value

    def close(self):
        if self.h:
            self.L.sqmc_gpu_spmv_free(self.h)
            self.h = None


def shell_sort_magnitude(a):
    """sqmc_shell_sort_magnitude: the reference's shell sort by magnitude, greatest first (shell_sort_real_rank1_int_rank1,
    generic_sort.f90:685-735; not stable).  Returns (sorted copy of a, its sign changed as a whole if the first element is negative;
    iorder, the 0-based positions in a that the sorted elements came from).  Runs on the host."""
    L = load_library()
    s = np.array(a, np.float64).ravel()
    if len(s) >= 2 ** 31:
        raise ValueError("more elements than iorder's 32-bit integers number")
    o = np.arange(len(s), dtype=np.int32)
    L.sqmc_shell_sort_magnitude.argtypes = [C.c_int64, C.c_void_p, C.c_void_p]
    _chk(L.sqmc_shell_sort_magnitude(len(s), _p(s), _p(o)))
    return s, o.astype(np.int64)


class Pt2StochasticPlan:
    """sqmc_gpu_hci_pt2_stochastic_prepare / _sample / _free: the samples of second_order_pt_alias (hci.f90:1314-1660) on the device.
    up, dn sorted by (up, dn); the plan borrows the context g: close it before g.  A context with time_sym is refused (the
    estimator is biased on time-reversal representatives): pass the determinant-basis expansion on one without."""

    def __init__(self, g, up, dn, coeffs, e_var, eps_pt, eps_pt_big, n_mc):
        self.L = g.L
        u, d, c = _u64(up), _u64(dn), _f64(coeffs)
        h = C.c_void_p()
        self.L.sqmc_gpu_hci_pt2_stochastic_prepare.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_double, C.c_double,
                                                               C.c_int32, C.c_void_p]
        self.L.sqmc_gpu_hci_pt2_stochastic_sample.argtypes = [C.c_void_p, C.c_int64] + [C.c_void_p] * 4
        self.L.sqmc_gpu_hci_pt2_stochastic_stats.argtypes = [C.c_void_p] * 5
        self.L.sqmc_gpu_hci_pt2_stochastic_free.argtypes = [C.c_void_p]
        self.h = None
        _chk(self.L.sqmc_gpu_hci_pt2_stochastic_prepare(g.h, len(u), _p(u), _p(d), _p(c), float(e_var), float(eps_pt), float(eps_pt_big), int(n_mc), C.byref(h)))
        self.h, self.g = h, g

    def sample(self, ids, counts):
        """ids: 0-based ascending positions of the distinct sampled determinants, counts: their multiplicities.
        Returns (the sample's value, connected determinants outside the variational space)."""
        i, w = np.ascontiguousarray(ids, np.int64), np.ascontiguousarray(counts, np.int64)
        if len(i) != len(w):
            raise ValueError("ids and counts differ in length")
        v, n = C.c_double(), C.c_int64()
        _chk(self.L.sqmc_gpu_hci_pt2_stochastic_sample(self.h, len(i), _p(i), _p(w), C.byref(v), C.byref(n)))
        return v.value, n.value

    def stats(self):
        """dict(n_alloc, capacity, last_raw, n_samples): (re)allocations of the connection buffers so far, what they hold, the raw
        connections of the latest sample, samples evaluated"""
        a = [C.c_int64() for _ in range(4)]
        _chk(self.L.sqmc_gpu_hci_pt2_stochastic_stats(self.h, *[C.byref(x) for x in a]))
        return dict(zip(("n_alloc", "capacity", "last_raw", "n_samples"), (x.value for x in a)))

    def close(self):
        if self.h:
            self.L.sqmc_gpu_hci_pt2_stochastic_free(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def _gpuchem_set_spawn_diagnostics(self, on=True):
    """sqmc_gpu_set_spawn_diagnostics: histograms of abs(weight_j)/tau and max / min weight ratios of every step from here on
    (off keeps the counts).  Walker lists and sums do not change; steps run un-pipelined while it is on."""
    self.L.sqmc_gpu_set_spawn_diagnostics.argtypes = [C.c_void_p, C.c_int32]
    _chk(self.L.sqmc_gpu_set_spawn_diagnostics(self.h, 1 if on else 0))


def _gpuchem_reset_spawn_diagnostics(self):
    self.L.sqmc_gpu_reset_spawn_diagnostics.argtypes = [C.c_void_p]
    _chk(self.L.sqmc_gpu_reset_spawn_diagnostics(self.h))


SPAWN_HIST_NBINS = 10001


def _gpuchem_spawn_diagnostics(self):
    """sqmc_gpu_get_spawn_diagnostics as a dict: nbins, bins / bins_hf / bins_single / bins_double (int64[nbins]; bin b of the
    reference is index b - 1, lower bound b - 1), max_ratio_by_level (float64[8], -1e99 where no proposal), max_ratio,
    max_ratio_level (-1: none), min_ratio (1e99: none), n_nan"""
    nb = C.c_int32()
    h = [np.zeros(SPAWN_HIST_NBINS, np.int64) for _ in range(4)]
    lv = np.zeros(8); mx, mn, ml, nn = C.c_double(), C.c_double(), C.c_int32(), C.c_int64()
    self.L.sqmc_gpu_get_spawn_diagnostics.argtypes = [C.c_void_p] * 11
    _chk(self.L.sqmc_gpu_get_spawn_diagnostics(self.h, C.byref(nb), _p(h[0]), _p(h[1]), _p(h[2]), _p(h[3]), _p(lv), C.byref(mx), C.byref(ml),
                                               C.byref(mn), C.byref(nn)))
    assert nb.value == SPAWN_HIST_NBINS
    return dict(nbins=nb.value, bins=h[0], bins_hf=h[1], bins_single=h[2], bins_double=h[3], max_ratio_by_level=lv, max_ratio=mx.value,
                max_ratio_level=ml.value, min_ratio=mn.value, n_nan=nn.value)


def _gpuchem_debug_bucket_boundaries(self, keys, B, kb=None, hint=None, kb_prev=None, pos_prev=None, scount=None, want_next=True):
    """sqmc_gpu_debug_bucket_boundaries (test door): the bucket-boundary kernel over ascending 32-bit keys.  kb, hint, kb_prev, pos_prev,
    scount: B + 1 words or None.  Returns (pos[B + 1] or None without kb, kb_out[B], hint_out[B]) -- the last two None unless want_next."""
    k = np.ascontiguousarray(keys, np.uint32)
    arrs = [None if a is None else np.ascontiguousarray(a, np.uint32) for a in (kb, hint, kb_prev, pos_prev, scount)]
    for a in arrs:
        if a is not None and len(a) != B + 1:
            raise ValueError("kb, hint, kb_prev, pos_prev and scount hold B + 1 words")
    pos = np.zeros(B + 1, np.uint32) if kb is not None else None
    kb_out, hint_out = (np.zeros(B, np.uint32), np.zeros(B, np.uint32)) if want_next else (None, None)
    self.L.sqmc_gpu_debug_bucket_boundaries.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int32] + [C.c_void_p] * 8
    _chk(self.L.sqmc_gpu_debug_bucket_boundaries(self.h, len(k), _p(k), int(B), *[None if a is None else _p(a) for a in arrs + [pos, kb_out, hint_out]]))
    return pos, kb_out, hint_out


GpuChem.debug_bucket_boundaries = _gpuchem_debug_bucket_boundaries
GpuChem.set_spawn_diagnostics = _gpuchem_set_spawn_diagnostics
GpuChem.reset_spawn_diagnostics = _gpuchem_reset_spawn_diagnostics
GpuChem.spawn_diagnostics = _gpuchem_spawn_diagnostics
GpuChem.hci_pt2 = _gpuchem_hci_pt2
GpuChem.hci_set_active_space = _gpuchem_hci_set_active_space
GpuChem.diag_update_batch = _gpuchem_diag_update_batch
GpuChem.hci_set_diag_update = _gpuchem_hci_set_diag_update
GpuChem.hci_connections_record = _gpuchem_hci_connections_record
GpuChem.one_rdm = _gpuchem_one_rdm
GpuChem.one_rdm_pt = _gpuchem_one_rdm_pt
GpuChem.two_rdm = _gpuchem_two_rdm
GpuChem.one_tdm = _gpuchem_one_tdm
GpuChem.two_tdm = _gpuchem_two_tdm
GpuChem.greens_function = _gpuchem_greens_function
GpuChem.rotate_integrals = _gpuchem_rotate_integrals
GpuChem.orbital_gradient = _gpuchem_orbital_gradient
GpuChem.one_index_transform = _gpuchem_one_index_transform
GpuChem.orbopt_plan = _gpuchem_orbopt_plan
