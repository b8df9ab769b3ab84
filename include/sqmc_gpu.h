/*
 * sqmc_gpu.h -- C ABI of libsqmc_gpu.so: the MI355X (gfx950) implementation of sqmc's
 * semistochastic walker step, deterministic-core matvec and HCI connection generation.
 *
 * This is the drop-in boundary: plain pointers and sizes, no C++/torch types.  A Fortran
 * host binds it with iso_c_binding (sqmc_amd/fortran/sqmc_gpu_mod.f90; INTEGRATION.md shows
 * the call sites to patch in the reference).  Each entry point cites the reference
 * interface it replaces, file:line relative to the reference's src/.
 *
 * Conventions (identical to the reference):
 *   - determinants: one 64-bit word per spin (n_det_words = 1, norb <= 64 this round); bit k
 *     <-> orbital k+1; walkers sorted by (up, then dn) as unsigned integers.  The reference
 *     splits its 128-bit dets into 2 x int64 on the wire (mpi_routines.f90:671-680); the
 *     low word is what is passed here, the high word must be zero.
 *   - CSR of the symmetric projector/Hamiltonian: "upper triangular" storage of
 *     more_tools.f90:3622-3670 -- row_counts(n), 1-based int64 column indices, fp64 values;
 *     every stored (i,m) with i != m is applied to both y(i) and y(m).
 *   - weights fp64; initiator in {0,1,2,3}; imp_distance in {-2,-1,0,1..127} as int8.
 *   - every function returns 0 on success; >0 are the reference's own stop conditions
 *     (see SQMC_ERR_*), <0 are library/HIP failures (text via sqmc_gpu_last_error()).
 *   - one context per process/GPU, driven by one host thread (the reference is
 *     single-threaded per MPI rank).
 */
#ifndef SQMC_GPU_H
#define SQMC_GPU_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct sqmc_gpu_ctx sqmc_gpu_ctx;

/* status codes > 0 mirror the reference's stop statements */
#define SQMC_OK 0
#define SQMC_ERR_MWALK 1          /* 'nwalk>MWALK'                    do_walk.f90:3684-3690 */
#define SQMC_ERR_SPAWN_OVERFLOW 2 /* spawn buffer full                mpi_routines.f90:2494 */
#define SQMC_ERR_NEG_DIAG 3       /* diagonal_factor<0 after equil.   do_walk.f90:3788     */
#define SQMC_ERR_NO_WALKERS 4     /* 'my_nwalk=0'                     do_walk.f90:2489     */
#define SQMC_ERR_IMP_BROKEN 5     /* 'locations of my imp broken'     do_walk.f90:2204     */
#define SQMC_ERR_BAD_ARG -1
#define SQMC_ERR_HIP -2
#define SQMC_ERR_UNSUPPORTED -3
#define SQMC_ERR_BREAKDOWN -4     /* sqmc_gpu_davidson: the iteration ended on something that is no eigen-solution (see there) */

/* RNG discipline.  REPLAY reproduces the reference's single rannyu stream draw for draw
 * (rannyu.f90:54-74 consumed in walker order, do_walk.f90:3577-3583, chemistry.f90:4391-4439,
 * do_walk.f90:7222-7230) and is meant for fixed-seed parity runs; COUNTER keys an
 * independent 48-bit stream on (seed, step, stage, entity) -- the walker index for the spawn
 * gate, the child index for a proposal, the determinant itself for the rounding draw -- so
 * that every stage is fully parallel and none needs a rank among the others.  Both give
 * reals k/2^48 like rannyu. */
#define SQMC_RNG_REPLAY 0
#define SQMC_RNG_COUNTER 1

/* Tables the reference builds in system_setup_chem / read_integrals / setup_orb_by_symm
 * (chemistry.f90:299-537, 538-869, 2461-2527) and keeps in module chemistry. */
typedef struct {
  int32_t norb, nup, ndn, n_core_orb;
  int32_t time_sym, z;              /* chemistry.f90:163-181; walks are over representatives */
  int32_t n_group;                  /* order of the abelian point group (<= 8)             */
  const int32_t *product_table;     /* [9*9], 1-based: product_table(i,j) at [i*9+j]       */
  const int32_t *orbital_symmetries;/* [norb+1], 1-based, after orbital reordering         */
  const int32_t *combine_2;         /* [(norb+2)*(norb+2)], 1-based, chemistry.f90:856-866 */
  int64_t n_integrals;              /* integral_index(norb+1,...,norb+1)                   */
  const double *integrals;          /* [n_integrals+1], 1-based packed array               */
  int32_t rng_mode;                 /* SQMC_RNG_*                                          */
  int32_t irand_seed[4];            /* stream-2 seed of input line 1, do_walk.f90:231,646  */
  int64_t mwalk;                    /* MWALK: capacity of the walker arrays                */
} sqmc_chem_cfg;

/* one process per GPU: select the device of this rank before creating a context (the
 * reference's cluster_init, mpi_routines.f90:766, has no device notion). */
int sqmc_gpu_set_device(int device);

/* replaces: system_setup_chem + init_move table setup.  Copies everything to HBM. */
int sqmc_gpu_init_chem(const sqmc_chem_cfg *cfg, sqmc_gpu_ctx **out);
/* Homogeneous electron gas in a plane-wave basis (hamiltonian_type 'heg'): the tables
 * system_setup_heg / generate_k_vectors build (heg.f90:168-215, 643-749).  k_vectors is the
 * reference's k_vectors(n_dim, norb) in its own (column-major) memory order, orbitals sorted by
 * |k| exactly as the reference sorts them; the walk then uses off_diagonal_move_heg
 * (heg.f90:1344-1598) and hamiltonian_heg (heg.f90:845-1011) in place of the chemistry pair. */
typedef struct {
  int32_t n_dim, norb, nup, ndn;
  double length_cell;
  const double *k_vectors;          /* [norb * n_dim] */
  int32_t rng_mode;
  int32_t irand_seed[4];
  int64_t mwalk;
} sqmc_heg_cfg;
int sqmc_gpu_init_heg(const sqmc_heg_cfg *cfg, sqmc_gpu_ctx **out);
/* Real-space Hubbard model on an l_x by l_y square lattice (hamiltonian_type 'hubbard2'): the
 * scalars read_hubbard takes from the deck (hubbard.f90:138-382: l_x, l_y, pbc, t, U, nup, ndn).
 * Site s (1-based) sits at x = mod(s-1, l_x)+1, y = (s-1)/l_x+1 and bit s-1 of a determinant
 * word; neighbours follow get_nbr (more_tools.f90:223-355).  The walk then uses
 * off_diagonal_move_hubbard (hubbard.f90:2992-3120) and hamiltonian_hubbard (1536-1644) as the
 * operator pair.  The energy estimator is the library's usual one over a determinant-list trial
 * wavefunction (the 'else' branch of energy_pieces_hubbard, 4514-4527, as a C(T) table); the
 * Gutzwiller/Slater trial functions of hubbard.f90 are host-side code outside this path.
 * The connection generator (sqmc_gpu_hci_connections, _slice, sqmc_gpu_hci_pt2) is find_connected_dets_hubbard
 * (hubbard.f90:5306-5457): sites ascending, at each site the up electron before the dn electron, per electron LEFT, RIGHT, UP,
 * DOWN, a hop where the neighbour is allowed and empty in that spin's string; the source itself in slot 0 (the reference puts it
 * last).  A hop is kept when |H c| > eps: every |H| is |t|, so the screen selects on |c| alone, and t = 0 leaves the own slot only.
 * A periodic direction of length 2 is refused: the reference's connected list counts that bond
 * twice while hamiltonian_hubbard counts it once.  On such a context the diagonal-update record, modes and batch, the active-space
 * masks, the stochastic-PT plan, hf_to_psit and the heat-bath and Cauchy-Schwarz set-up return SQMC_ERR_UNSUPPORTED. */
typedef struct {
  int32_t l_x, l_y, pbc, nup, ndn;
  double t, U;
  int32_t rng_mode;
  int32_t irand_seed[4];
  int64_t mwalk;
} sqmc_hubbard_cfg;
int sqmc_gpu_init_hubbard(const sqmc_hubbard_cfg *cfg, sqmc_gpu_ctx **out);
/* Hubbard model in its plane-wave basis on a periodic l_x by l_y lattice (hamiltonian_type 'hubbardk'; space_sym = .true.: sqmc_gpu_set_hubbardk_space_sym):
 * hubbard.f90:2179-2324 (generate_k_vectors), 2866-2924 (hamiltonian_hubbard_k), 3649-3848 (off_diagonal_move_hubbard_k),
 * 5462 (find_connected_dets_hubbard_k).  The orbital table arrives as data in the reference's orbital order, as
 * sqmc_gpu_init_heg takes its plane waves: k_vectors is the reference's k_vectors(2, nsites) (int32, two per orbital, units of
 * pi / L), k_energies its k_energies(nsites).  The library builds the momentum -> orbital lookup itself (nsites entries; the
 * reference's kmap).  sys_type 3: H_ii = U/nsites * nup * ndn + the occupied orbitals' energies; every off-diagonal element is
 * +-U/nsites between determinants one up and one dn electron apart with the total momentum conserved modulo (2 l_x, 2 l_y);
 * the proposal draws random_int(nup), random_int(ndn), random_int(nsites - nup) in that order.
 * The connection generator (sqmc_gpu_hci_connections, _slice, sqmc_gpu_hci_pt2) loops up electrons x dn electrons x empty up
 * orbitals, ascending, and keeps a connection when |H c| > eps: every |H| is U/nsites, so the screen selects on |c| alone.
 * Refused: l_x * l_y > 64; a length of 2 (the double bond sqmc_gpu_init_hubbard refuses); both lengths 1; nup or ndn outside
 * 1 .. nsites - 1 (the move needs one electron of each spin and a hole); a k table that is not exactly one orbital per lattice
 * momentum modulo (2 l_x, 2 l_y).  Chains (one length 1, the other >= 3) are supported.  On such a context the diagonal-update
 * modes, the active-space masks, the stochastic-PT plan and hf_to_psit return SQMC_ERR_UNSUPPORTED, as for hubbard2. */
typedef struct {
  int32_t l_x, l_y, nup, ndn;
  double t, U;
  const int32_t *k_vectors;         /* [2 * nsites] */
  const double *k_energies;         /* [nsites] */
  int32_t rng_mode;
  int32_t irand_seed[4];
  int64_t mwalk;
} sqmc_hubbardk_cfg;
int sqmc_gpu_init_hubbardk(const sqmc_hubbardk_cfg *cfg, sqmc_gpu_ctx **out);
/* space_sym = .true. for hubbardk (read_hubbard, hubbard.f90:181-208): the walk lives on the representatives of the orbits of the
 * determinants under C4 x lattice reflection x spin inversion (16 elements), in the sector z (spin inversion), p (reflection), C4-A1.
 * replaces: generate_fourfold_k_configs_efficient (more_tools.f90:4670-4819: the 16 images with their phases, the representative = the
 * smallest image by (up, dn), phase_w_rep, norm, num_distinct), hamiltonian_hubbard_k_space_sym (hubbard.f90:2927-2989), the space_sym
 * branch of off_diagonal_move_hubbard_k (3771-3817: the child is replaced by its representative, proposal_prob_inv / nnzero, weight 0 onto
 * a determinant of norm 0, onto the parent's own orbit, or with nnzero = 0; the same three random_int draws) and the closing block of
 * find_connected_dets_hubbard_k (5611-5627).  c4_map is the reference's c4_map(3, nsites) as it lies in memory (three entries per orbital)
 * and reflection_map its reflection_map(nsites), both 1-based, as create_kspace_sym_maps (more_tools.f90:4209-4310) builds them.
 * After this call every element (sqmc_gpu_hamiltonian_batch, H_ii of the walk), every move and every connection of the context is the
 * one between orbit sums; a bra that is not a representative stands for its representative, and an element with a determinant of norm 0
 * is 0.  The connection generator emits every raw child as (its representative, its term of the symmetrised element times c): the
 * deduplication sums them; children in the source's own orbit land on the source's slot, which holds the plain diagonal in diag_mode 1
 * (together: the symmetrised H_ii); the eps screen stays on the raw term |U/nsites c|.
 * Refused (SQMC_ERR_UNSUPPORTED): a context that is not hubbardk, l_x /= l_y or odd l, nup /= ndn.  SQMC_ERR_BAD_ARG: |z| or |p| /= 1; maps
 * that are not permutations, do not preserve k_energies or do not compose as C4 and a reflection; a context that already holds walkers, a
 * projector or a C(T) table.  With space_sym set, sqmc_gpu_upload_walkers and sqmc_gpu_set_ct_table refuse (SQMC_ERR_BAD_ARG) a determinant
 * that is not its own representative or whose norm is 0 (sqmc_gpu_set_projector takes a matrix without determinants: its rows are the
 * uploaded walkers with imp_distance 0, which are checked), and sqmc_gpu_hci_pt2, sqmc_gpu_build_sparse_ham and sqmc_gpu_build_spmv_plan
 * return SQMC_ERR_UNSUPPORTED in addition to what a hubbardk context refuses anyway. */
int sqmc_gpu_set_hubbardk_space_sym(sqmc_gpu_ctx *ctx, int32_t z, int32_t p, const int32_t *c4_map, const int32_t *reflection_map);
/* per determinant of a list (any determinants of nup + ndn electrons, representatives or not): images_up / images_dn [16 n] and phases [16 n]
 * in the reference's order (image k of determinant i at [16 i + k]), the representative, phase_w_rep, norm and num_distinct
 * (0 when the norm vanishes).  What symmetry_reduce_hubbardk (hubbard.f90:9061) needs to reduce a determinant list. */
int sqmc_gpu_hubbardk_sym_images(sqmc_gpu_ctx *ctx, int64_t n, const uint64_t *up, const uint64_t *dn, uint64_t *images_up, uint64_t *images_dn,
                                 int32_t *phases, uint64_t *rep_up, uint64_t *rep_dn, int32_t *phase_w_rep, double *norm, int32_t *num_distinct);
int sqmc_gpu_finalize(sqmc_gpu_ctx *ctx);
const char *sqmc_gpu_last_error(void);

/* proposal_method 'fast_heatbath': the tables setup_efficient_heatbath builds when run_type /= hci (chemistry.f90:1002-1225),
 * handed over exactly as the reference holds them (module variables of chemistry.f90:52-75; Fortran column-major order, the
 * four-index arrays and their alias tables 1-D and single precision, indexed by same_index / opposite_index, 9154-9193).
 * After this call sqmc_gpu_step spawns with off_diagonal_move_chem_efficient_heatbath (5086-5347) instead of
 * off_diagonal_move_chem: every child may add TWO walkers (a single excitation larger than all its doubles together comes
 * back with a double, do_walk.f90:3604-3611 -> add_walker 7584-7697), so a step needs room for 2 x children spawned walkers.
 * Both RNG disciplines (REPLAY: one lane runs every proposal to follow the stream).  Systems for which check_heatbath_unbiased (9330-9375) fails are the caller's to refuse, as the
 * reference does (1215-1223).  tests/golden/README_heatbath.md records what parity is defined against. */
typedef struct {
  int32_t norb, reserved;
  const double *one_orbital_probabilities;                 /* (norb) */
  const double *two_orbital_probabilities;                 /* (2 norb, 2 norb) */
  const double *three_orbital_probabilities_same_spin;     /* (norb, norb, norb), normalised over the last index */
  const double *three_orbital_probabilities_opposite_spin;
  const int32_t *J_three_orbital_probabilities_same_spin, *J_three_orbital_probabilities_opposite_spin;   /* alias tables, (norb, norb, norb) */
  const double *q_three_orbital_probabilities_same_spin, *q_three_orbital_probabilities_opposite_spin;
  int64_t size_same, size_opposite;                        /* same_index(norb,norb,norb,norb), opposite_index(norb,norb,norb,norb) */
  const float *four_orbital_probabilities_same_spin, *four_orbital_probabilities_opposite_spin;
  const int32_t *J_four_orbital_probabilities_same_spin, *J_four_orbital_probabilities_opposite_spin;
  const float *q_four_orbital_probabilities_same_spin, *q_four_orbital_probabilities_opposite_spin;
  const double *Htot_same;                                 /* (combine_2_indices(norb, norb), norb) */
  const double *Htot_opposite;                             /* (norb, norb, norb) */
} sqmc_heatbath_tables;
int sqmc_gpu_set_heatbath_tables(sqmc_gpu_ctx *ctx, const sqmc_heatbath_tables *t);
/* replaces: setup_efficient_heatbath for run_type /= hci (chemistry.f90:1002-1225) with setup_alias (more_tools.f90:5603-5722) and
 * check_heatbath_unbiased (9330-9375): the library builds the tables itself -- |H_ijkl| of all orbital quadruples on the device, the
 * partial sums, normalisations and alias tables in the reference's loop order and precisions -- and installs them as
 * sqmc_gpu_set_heatbath_tables would.  *is_heatbath_unbiased = (max(nup, ndn) > number of orbitals of unique symmetry); when it is 0
 * the reference stops ("Heatbath may be biased for this system!", 1219) and nothing is installed.  sqmc_gpu_get_heatbath_tables hands
 * out the library's host copies (the reference's layout; valid until the next setup call or sqmc_gpu_finalize). */
int sqmc_gpu_setup_efficient_heatbath(sqmc_gpu_ctx *ctx, int32_t *is_heatbath_unbiased);
int sqmc_gpu_get_heatbath_tables(sqmc_gpu_ctx *ctx, sqmc_heatbath_tables *t, int32_t *n_orb_uniq_sym);
/* n proposals of off_diagonal_move_chem_efficient_heatbath, each from its own rannyu state seeds[4 i .. 4 i + 3] (test door, like
 * sqmc_gpu_propose_batch): det_j and weight_j = -tau H_ij / p of the two slots of proposal i at [2 i] and [2 i + 1] (weight 0: no move). */
int sqmc_gpu_propose_heatbath_batch(sqmc_gpu_ctx *ctx, int64_t n, double tau, const uint64_t *up, const uint64_t *dn, const int32_t *seeds,
                                    uint64_t *det_j_up, uint64_t *det_j_dn, double *weight_j, int32_t *seeds_after);

/* proposal_method 'CauchySchwarz' (chem only; time_sym = 0 or 1, z = +-1).
 * replaces: setup_orb_by_symm's CauchySchwarz block (chemistry.f90:2505-2523): sqrt_integrals(i,j) = sqrt((ij|ij)), cs_sqrt_orb and
 * sym_sum_cs_sqrt, built from the context's integrals in the reference's loop order.  Like the reference it stops on an exchange
 * integral below -1e-6 (a default-real literal: -9.999999974752427e-07) -- SQMC_ERR_BAD_ARG, last error "Negative integrals!", nothing
 * changed -- and overwrites every slightly negative one with 0 in the integrals themselves (host and device), which H then uses
 * everywhere; *n_clamped (may be null) counts them.  As in system_setup_chem, this comes before anything built from H: with a projector,
 * C(T), Psi_T tables, HCI tables or walkers present it fails with SQMC_ERR_BAD_ARG.  Fast heat-bath and Cauchy-Schwarz exclude each other
 * on one context (the second set-up fails with SQMC_ERR_BAD_ARG, the first stays).  After this call sqmc_gpu_step / _run and the sharded
 * steps spawn with off_diagonal_move_chem_cauchySchwarz (2530-4233, do_walk.f90:3613-3614, 3937-3938), one walker slot per child,
 * both RNG disciplines; the intrinsic random_number draws of the reference come from the walk's own stream
 * (tests/golden/README_cauchyschwarz.md).  With time_sym the move ends as 4093-4162 do: the second pathway through the time-reversed
 * det_j from the Cauchy-Schwarz arm of is_connected_chem (tests/golden/README_cauchyschwarz_time_sym.md) and det_j replaced by its
 * representative (up <= dn).  hf_to_psit with this proposal is refused (SQMC_ERR_UNSUPPORTED). */
int sqmc_gpu_setup_cauchy_schwarz(sqmc_gpu_ctx *ctx, int32_t *n_clamped);
/* n proposals of off_diagonal_move_chem_cauchySchwarz (chemistry.f90:2530-4233), each from its own rannyu state seeds[4 i .. 4 i + 3]
 * (test door, like sqmc_gpu_propose_batch): det_j and weight_j = -tau H_ij / proposal_prob (4204); weight 0 and det_j = det_i where
 * the reference returns early or a cumulative search falls through.  With time_sym, det_j is the representative and weight_j the
 * combined weight of both pathways (4093-4162). */
int sqmc_gpu_propose_cauchy_schwarz_batch(sqmc_gpu_ctx *ctx, int64_t n, double tau, const uint64_t *up, const uint64_t *dn, const int32_t *seeds,
                                          uint64_t *det_j_up, uint64_t *det_j_dn, double *weight_j, int32_t *seeds_after);

/* replaces: dtm_hb / pq_ind / pq_count built by setup_efficient_heatbath (chemistry.f90:900-993).
 * hb_r/hb_s/hb_absH: n_hb records sorted by descending absH inside each (p,q) class;
 * pq_ind (1-based start) / pq_count indexed by combine_2_indices(p,q) in [1, n_pq]. */
int sqmc_gpu_set_hb_tables(sqmc_gpu_ctx *ctx, int64_t n_hb, const int32_t *hb_r, const int32_t *hb_s,
                           const double *hb_absH, int32_t n_pq, const int64_t *pq_ind,
                           const int32_t *pq_count, double max_double);

/* replaces: minus_tau_H_indices / _nonzero_elements / _values (common_imp.f90:14-15) as
 * consumed at do_walk.f90:2262; scale = the tau_ratio rescale of do_walk.f90:2179,2919. */
int sqmc_gpu_set_projector(sqmc_gpu_ctx *ctx, int64_t n_imp, int64_t nnz, const int64_t *row_counts,
                           const int64_t *indices, const double *values);
int sqmc_gpu_scale_projector(sqmc_gpu_ctx *ctx, double ratio);

/* replaces: psi_t_connected_dets_up/dn, psi_t_connected_e_loc_num/den (common_psi_t.f90:20-32),
 * sorted by (up,dn), searched by binary_search_list_and_update (more_tools.f90:4041-4098). */
int sqmc_gpu_set_ct_table(sqmc_gpu_ctx *ctx, int64_t n, const uint64_t *up, const uint64_t *dn,
                          const double *e_num, const double *e_den);

/* hf_to_psit = .true. (input line do_walk.f90:378; "replace HF with psi_T for 1st state"): the step variant in which the first basis
 * state is the trial wave function, moves to and from it are deterministic and all determinants of C(T) stay in the walker list
 * (do_walk.f90:1056-1116, 1267-1300, 2272-2320, 2394-2462, 2701-2722, 3574, 3676, 5268-5307, 6484-6833, 7206-7254).
 * Call after sqmc_gpu_set_ct_table and sqmc_gpu_set_projector, before sqmc_gpu_upload_walkers:
 *   - the projector is the deterministic-space matrix as generate_sparse_ham_*_upper_triangular builds it with hf_to_psit
 *     (chemistry.f90:7885-7897, 7926-7933: no first row and column, the (1,1) element stored as 0), times -tau;
 *   - psit_ct_index[k] (1-based, increasing): where dets_up/dn_psi_t(k), Psi_T in label order (do_walk.f90:1258), lies in the C(T)
 *     list -- my_locations_of_psit (1849-1886); the first must be 1;  cdet_psi_t[k] its coefficient;
 *   - diag_elems[n_ct]: H_ii of the C(T) determinants outside the deterministic space, 0 inside (1091-1116);
 *   - the walker list is [the n_ct determinants of C(T) in order | the survivors outside C(T) in order]: upload takes it so
 *     (at the start: C(T) alone, do_walk.f90:1267-1300, imp_distance 0 inside the deterministic space and -2 elsewhere) and
 *     download returns it so.  The deterministic space must lie inside C(T) and only the first state may be a permanent initiator,
 *     as in the reference's own set-up.
 * sum_order: 1 = the step's three long sums (first row over C(T), first row over Psi_T, T^-1) through a fixed 64-ary tree;
 * 0 = left to right as the reference's loops run (one lane: slow).  One rank, COUNTER or REPLAY discipline, uniform proposal
 * (over ranks: sqmc_gpu_set_hf_to_psit_shard below).
 * tests/golden/README_hf_to_psit.md records what parity is defined against (the reference's merge for this variant cannot run as written). */
int sqmc_gpu_set_hf_to_psit(sqmc_gpu_ctx *ctx, int64_t n_psit, const int64_t *psit_ct_index, const double *cdet_psi_t,
                            const double *diag_elems, int32_t sum_order);

/* walker SoA of common_walk.f90:5-18.  perm_sign(i) = sign_permanent_initiator of walker i
 * if initiator(i)==3 else 0 (the reference keeps the signs in sorted-walker order,
 * do_walk.f90:1150,2593-2594; here the sign travels with its walker). */
int sqmc_gpu_upload_walkers(sqmc_gpu_ctx *ctx, int64_t n, const uint64_t *up, const uint64_t *dn,
                            const double *wt, const int8_t *imp_distance, const int8_t *initiator,
                            const int8_t *perm_sign, const double *matrix_elements,
                            const double *e_num, const double *e_den);
int sqmc_gpu_num_walkers(sqmc_gpu_ctx *ctx, int64_t *n);
int sqmc_gpu_download_walkers(sqmc_gpu_ctx *ctx, int64_t cap, int64_t *n, uint64_t *up, uint64_t *dn,
                              double *wt, int8_t *imp_distance, int8_t *initiator,
                              double *matrix_elements, double *e_num, double *e_den);

/* by-value scalars of one MC step, do_walk.f90:2171-2934 */
typedef struct {
  double tau, e_trial, reweight_factor_inv, r_initiator, min_wt, always_spawn_cutoff_wt;
  int32_t initiator_power, initiator_min_distance, c_t_initiator, semistochastic, reached_w_abs_gen;
  int32_t reserved;
} sqmc_step_params;

/* out_stats[16]: 0 w_gen  1 w_abs_gen  2 e_den_gen  3 e_num_gen  4 w_perm_initiator_gen
 *   5 nwalk  6 w_abs_gen_imp  (the 7 reduced values of do_walk.f90:2689-2725)
 *   7 nwalk_before_merge  8 w2_gen  9 e_num2  10 e_den2  11 e_num_abs  12 e_den_abs
 *   13 e_num_e_den (the my_*_cum increments, 2670-2679)  14 w_abs_before_merge
 *   15 number of off-diagonal proposals made.
 * replaces: the move loop, deterministic projection, sort, merge, reduce, reweight and
 * estimator sums of do_walk.f90:2216-2487 and 2573-2790 (semistochastic chem, ncores=1). */
int sqmc_gpu_step(sqmc_gpu_ctx *ctx, const sqmc_step_params *p, double out_stats[16]);
/* Population control around the step, as the reference's walk loop does it on the host:
 * tau / r_initiator ramp until w_abs_gen_target is first reached (do_walk.f90:2175-2184,
 * 2913-2923, with the projector rescaled by tau_ratio), e_est from the cumulated sums,
 * e_trial and reweight_factor_inv (do_walk.f90:2880-2901).  The first n_equil steps count as
 * equilibration (iblkk <= ntimes_nblk_eq*nblk_eq in the reference). */
typedef struct {
  double tau_sav, tau, tau_prev;          /* input tau; current (ramped) tau; tau of the previous step */
  double e_trial, e_est;
  double w_abs_gen_target, w_abs_gen;     /* target; w_abs_gen of the last step (set to the initial sum|w| before the first) */
  double r_initiator_sav, r_initiator, initiator_rescale_power;
  double population_control_exponent;
  double reweight_factor_inv, reweight_factor_inv_max;
  double e_num_cum, e_den_cum;            /* sums of e_num_gen*sign(e_den_gen), |e_den_gen| */
  double min_wt, always_spawn_cutoff_wt;
  int32_t reached_w_abs_gen, initiator_power, initiator_min_distance, c_t_initiator, semistochastic, reserved;
  int64_t istep, n_equil;
} sqmc_popctl;

/* replaces: the body of "do istep=1,nstep" (do_walk.f90:2171-2934) for nsteps consecutive steps
 * without returning to the caller in between: sqmc_gpu_step + the scalar updates above.
 * stats (may be NULL) receives the 16 per-step values of every step (nsteps*16 doubles);
 * totals[16] their sums over the nsteps steps.  pc is updated in place. */
int sqmc_gpu_run(sqmc_gpu_ctx *ctx, sqmc_popctl *pc, int64_t nsteps, double *stats, double totals[16]);

/* replaces: merge_sort2_up_dn + merge_original_with_spawned2 + reduce_my_walker and the estimator
 * sums, do_walk.f90:2364-2487, 2573-2790, as one call for a host that produces its spawns itself:
 * the n_spawn walkers (in creation order; weight 0 = no walker; imp_distance / initiator as
 * move_uniform2 sets them, do_walk.f90:3700-3727) are appended behind the resident walkers, then
 * sort, annihilation with the initiator rules, stochastic rounding, reweighting and the sums of
 * sqmc_gpu_step.  out_stats as in sqmc_gpu_step (entry 15 = 0). */
int sqmc_gpu_annihilate(sqmc_gpu_ctx *ctx, const sqmc_step_params *p, int64_t n_spawn, const uint64_t *up, const uint64_t *dn,
                        const double *wt, const int8_t *imp_distance, const int8_t *initiator, double out_stats[16]);

/* ---- multi-rank sharding: one process per GPU, walkers owned by hash(det) mod nranks, as the
 * reference shards them over MPI ranks (get_det_owner, mpi_routines.f90:419-445).  The library
 * does no communication itself: the step is cut at the reference's two exchange points and the
 * host moves device buffers with its collective library (RCCL through torch.distributed in
 * sqmc_amd/host.py; MPI in the reference):
 *   shard_begin   gate, death/clone, spawn; owned deterministic-space weights -> x_global
 *     [host: all-reduce SUM of x_global]                      (mpi_redscatt, do_walk.f90:2259-2260)
 *   shard_pack    owned rows of the projection; spawns bucketed by owner into 32-byte records
 *     [host: all-to-all of the counts, then of the records]   (mpi_sendnewwalks, do_walk.f90:2237)
 *   shard_finish  received records appended; sort, annihilation, rounding, estimator sums
 *     [host: all-reduce SUM of out_stats[0..6]]               (mpi_allred, do_walk.f90:2778)
 * set_projector takes the GLOBAL projector on every rank; shard_config gives, for the k-th
 * deterministic-space walker this rank owns (in its sorted order), its row in that matrix.
 *
 * Proposal: the sharded steps spawn with the context's proposal -- uniform, CauchySchwarz, or fast_heatbath once its tables are set
 * (sqmc_gpu_set_heatbath_tables / sqmc_gpu_setup_efficient_heatbath, before or after sqmc_gpu_shard_config; COUNTER discipline only).
 * A fast_heatbath child holds TWO walker slots, the single and the double excitation of one proposal (do_walk.f90:3604-3611), so a
 * step of nch children has spc * nch spawn slots, spc = 2 (1 for every other proposal):
 *   - capacity: nwalk + spc * nch > MWALK stops the step with SQMC_ERR_MWALK ("nwalk>MWALK"), as in sqmc_gpu_step, also for a
 *     pipelined head of sqmc_gpu_shard_run; with a communicator the stop is collective;
 *   - records: every slot that holds a walker becomes one 32-byte record, routed by the owner of ITS determinant (the two slots
 *     of a child may go to different ranks); empty slots are neither counted in send_counts nor sent, so a step sends at most
 *     spc * nch records.  Inside a destination the records keep slot order.  sqmc_gpu_shard_pack with cap_records smaller than
 *     the records to send gives SQMC_ERR_SPAWN_OVERFLOW before anything is written.  The in-library step stages all slots, the
 *     empty ones behind the last rank's, so its check is the conservative one: spc * nch slots against its staging buffer of
 *     MWALK records (which the capacity rule above already guarantees);
 *   - *n_children and out_stats[15] count children (proposals), not slots.
 * fast_heatbath together with sqmc_gpu_set_hf_to_psit_shard is refused (SQMC_ERR_UNSUPPORTED), in either order of the calls. */
int sqmc_gpu_det_owner(sqmc_gpu_ctx *ctx, int64_t n, const uint64_t *up, const uint64_t *dn, int32_t nranks, int32_t *owner);
/* Which hash decides ownership.  0 (default): a mix of the determinant's sort key (cheapest).  1: the reference's own
 * get_det_owner -> hash -> djb_hash (mpi_routines.f90:419-445, 257-289, 354-379) bit for bit, so that ranks running the
 * reference and ranks running this library agree on who owns a determinant.  Call before distributing walkers. */
int sqmc_gpu_set_owner_hash(sqmc_gpu_ctx *ctx, int32_t mode);
int sqmc_gpu_shard_config(sqmc_gpu_ctx *ctx, int32_t rank, int32_t nranks, int64_t n_imp_local, const int32_t *global_row);
int sqmc_gpu_shard_begin(sqmc_gpu_ctx *ctx, const sqmc_step_params *p, double *x_global_dev, int64_t *n_children);
int sqmc_gpu_shard_pack(sqmc_gpu_ctx *ctx, const sqmc_step_params *p, const double *x_global_dev, uint64_t *send_dev,
                        int64_t cap_records, int64_t *send_counts);
int sqmc_gpu_shard_finish(sqmc_gpu_ctx *ctx, const sqmc_step_params *p, const uint64_t *recv_dev, int64_t n_recv, double out_stats[16]);

/* The same sharded step with the three exchanges issued by the library itself over RCCL/xGMI
 * (replaces mpi_allred of the deterministic weights do_walk.f90:2259-2260, mpi_snd_list /
 * mpi_sendnewwalks mpi_routines.f90:1147-1270, and the mpi_allred of the sums
 * do_walk.f90:2778-2790).  Rank 0 obtains an id with sqmc_gpu_comm_unique_id and hands it to the
 * other ranks by any means (MPI_Bcast in the reference's build); every rank then calls
 * sqmc_gpu_comm_init after sqmc_gpu_shard_config.  sqmc_gpu_shard_step = begin + all-reduce +
 * pack + all-to-all + finish + all-reduce: out_stats[0..6] are sums over all ranks,
 * out_stats[7..15] stay local.  sqmc_gpu_shard_run is sqmc_gpu_run over sharded steps (every
 * rank carries the same population-control state, as the reference's ranks do).  Once a
 * communicator is attached, sqmc_gpu_shard_finish also all-reduces; use either the three-phase
 * calls without a communicator or shard_step with one. */
#define SQMC_COMM_ID_BYTES 128

/* hf_to_psit over ranks (do_walk.f90:1808-1886, 2272-2288, 2304-2320, 2394-2462, 2701-2722): the step variant of
 * sqmc_gpu_set_hf_to_psit on a sharded walk, chem and HEG, uniform proposal, COUNTER discipline.  Call after sqmc_gpu_shard_config
 * (with the global projector of sqmc_gpu_set_hf_to_psit and the global C(T) table set on every rank), before sqmc_gpu_upload_walkers:
 *   - ct_index[n_ct_local] (1-based, increasing): the C(T) determinants this rank owns, as positions in the C(T) list
 *     (my_ndet_psi_t_connected); they sit at the head of its walker list in C(T) order; diag_elems[n_ct_local] as for one rank;
 *   - psit_slot[n_psit_local] (1-based in that share, increasing): my_locations_of_psit; psit_mask[k]: the index of the entry in
 *     Psi_T in label order (ndet_psit_mask); cdet_psi_t[n_psit]: all of Psi_T's coefficients;
 *   - the first state (C(T)'s and Psi_T's first determinant) is at slot 1 of its owner (iown_first = iown_psit1); a share may be empty.
 * Exchanges, beside the existing three: x_global is n_imp + 2*nranks doubles -- slots n_imp + r and n_imp + nranks + r carry rank r's
 * partials of the first row over C(T) and over Psi_T, zero from every other rank, so its all-reduce is exact -- and, after the
 * merge, one all-reduce (SUM) of nranks + 1 doubles: rank r's partial of T^-1's sum in entry r, the owner's weight of the first
 * state in entry nranks.  With a communicator the library issues it; without one, finish each step with
 * sqmc_gpu_shard_finish_psit, which writes the vector to reduce_buf_dev (device, nranks + 1 doubles), synchronises, calls
 * allreduce(reduce_buf_dev, nranks + 1, user) -- which must return 0 once the buffer holds the sum over ranks -- and goes on.
 * Sum order: inside a rank, the local terms through the fixed 64-ary tree (sum_order 1) or left to right (0), as for one rank;
 * across ranks, the partials added in rank order.  One rank is therefore the one-rank step bit for bit, and every rank sees the
 * same bits.  sqmc_gpu_shard_run runs this variant unpipelined.  Refused: fast_heatbath tables, the Hubbard model. */
typedef int (*sqmc_allreduce_fn)(double *buf_dev, int64_t n, void *user);
int sqmc_gpu_set_hf_to_psit_shard(sqmc_gpu_ctx *ctx, int64_t n_ct_local, const int64_t *ct_index, const double *diag_elems,
                                  int64_t n_psit_local, const int64_t *psit_slot, const int64_t *psit_mask, int64_t n_psit,
                                  const double *cdet_psi_t, int32_t sum_order);
int sqmc_gpu_shard_finish_psit(sqmc_gpu_ctx *ctx, const sqmc_step_params *p, const uint64_t *recv_dev, int64_t n_recv,
                               double *reduce_buf_dev, sqmc_allreduce_fn allreduce, void *user, double out_stats[16]);
int sqmc_gpu_comm_unique_id(uint8_t id[SQMC_COMM_ID_BYTES]);
int sqmc_gpu_comm_init(sqmc_gpu_ctx *ctx, const uint8_t id[SQMC_COMM_ID_BYTES]);
/* number of ranks RCCL itself reports for the communicator (ncclCommCount; the reference's ncores, mpi_routines.f90:310) */
int sqmc_gpu_comm_size(sqmc_gpu_ctx *ctx, int32_t *nranks);
int sqmc_gpu_shard_step(sqmc_gpu_ctx *ctx, const sqmc_step_params *p, double out_stats[16]);
int sqmc_gpu_shard_run(sqmc_gpu_ctx *ctx, sqmc_popctl *pc, int64_t nsteps, double *stats /* nsteps*16 or NULL */, double totals[16]);
/* diagnostics: where the HOST spent the wall clock of the sqmc_gpu_shard_step calls since the last reset, in microseconds summed over
 * *steps completed steps: us[0] head (gate, spawn and death/clone enqueued or taken over from the pipelined head, until the child count is
 * known), us[1] exchange (projection all-reduce, bucketing by owner, pack, all-gather of the send counts until the host has read them,
 * grouped send/receive enqueued), us[2] tail (unpack, sort and annihilation enqueued, until the all-reduced sums are read; the next
 * step's head is enqueued in here), us[3] the part of all three spent waiting for a word the GPU writes.  What a scaling run needs to
 * explain itself: kernel time hides inside the waits, link latency inside us[1] and us[2]. */
int sqmc_gpu_shard_time_split(sqmc_gpu_ctx *ctx, double us[4], int64_t *steps, int32_t reset);

/* RNG state of the REPLAY stream (savern / setrn, rannyu.f90:11-21,77-87) */
/* How many steps took the short-list tail (block-local partition + one annihilation kernel per key range, no global sort) and
 * how many of those had to be re-run through the radix tail because a key range outgrew its block (diagnostics, tests). */
int sqmc_gpu_tail_stats(sqmc_gpu_ctx *ctx, int64_t *bucket_steps, int64_t *bucket_retries);
/* Which tail the LAST step (sqmc_gpu_step, a step of sqmc_gpu_run, sqmc_gpu_annihilate, a sharded finish) took (diagnostics, tests):
 * info[0] 0 = radix tail, 1 = short-list (bucket) tail, 2 = bucket tail that gave up and was re-run through the radix tail;
 * info[1] sorted slots per thread of the annihilation kernel that produced the list (2, 3 or 4; 0 for the bucket kernel and for a
 *         step that is not semistochastic);  info[2] 1 if only the spawns were sorted and merged into the ordered residents;
 * info[3] 1 if sort keys and walker indices share one 64-bit word (keys of at most 32 bits), 0 for the two-array layout. */
int sqmc_gpu_last_tail(sqmc_gpu_ctx *ctx, int32_t info[4]);
/* A host that runs the walk in blocks (nstep steps, then its block statistics: do_walk.f90:2171 inside the iblk loop, 2086-3300)
 * calls sqmc_gpu_run once per block.  With chained runs on, the last step of a call enqueues the head (gate, child offsets, spawn)
 * of the first step of the NEXT call behind its own tail, as every other step of the call does for its successor, so the GPU keeps
 * working while the host does its block bookkeeping (the first step of a call costs 0.135 instead of 0.075 ms otherwise).  The
 * head is forgotten, at the cost of one stream synchronisation, if anything but a step with the same tau / cutoff / mode comes
 * next (walkers uploaded or downloaded, projector rescaled, tables of either heat-bath kind set, hf_to_psit set, RNG reset, chaining switched off, finalize).  The same holds for a host that
 * calls sqmc_gpu_step itself, step by step (its own work between steps, as in the reference's loop): with chaining on, every step past the
 * target population enqueues its successor's head.  Single-GPU steps only. */
int sqmc_gpu_set_chained_runs(sqmc_gpu_ctx *ctx, int32_t on);
/* diagnostics: wall-clock time (microseconds) and index of the four slowest steps of the last sqmc_gpu_run / sqmc_gpu_shard_run
 * call -- a step that waited for the host (scheduling, a rerun through the radix tail) stands out here */
int sqmc_gpu_slowest_steps(sqmc_gpu_ctx *ctx, double us[4], int64_t step[4]);
int sqmc_gpu_get_rng(sqmc_gpu_ctx *ctx, int32_t seed[4]);
int sqmc_gpu_set_rng(sqmc_gpu_ctx *ctx, const int32_t seed[4]);

/* replaces: fast_sparse_matrix_multiply_upper_triangular (more_tools.f90:3622-3670) as
 * called from davidson_sparse (more_tools.f90:2115,2188).  prepare once per matrix
 * (converts to int32 full CSR in HBM), apply per matvec.  x/y are host pointers unless
 * on_device != 0. */
typedef struct sqmc_spmv_plan sqmc_spmv_plan;
int sqmc_gpu_spmv_prepare(int64_t n, const int64_t *row_counts, const int64_t *indices,
                          const double *values, sqmc_spmv_plan **plan);
int sqmc_gpu_spmv_apply(sqmc_spmv_plan *plan, const double *x, double *y, int on_device);
int sqmc_gpu_spmv_free(sqmc_spmv_plan *plan);
/* The lowest n_states eigenpairs of the plan's matrix by the diagonally preconditioned Davidson of davidson_sparse
 * (more_tools.f90:2018-2244; davidson_sparse_single :3056-3230), every vector resident on the device.  diag[n]: the diagonal (the
 * preconditioner, as sqmc_gpu_build_spmv_plan returns it); v0: n x n_states start vectors, column-major (initial_vector), or NULL for
 * unit vectors on the first rows (more_tools.f90:3113-3114: the HF determinant when it is listed first); tol: the reference's
 * epsilon = 1e-10 on the eigenvalues.  Out: evals[n_states], evecs[n x n_states] column-major (largest component of the small
 * problem's eigenvector positive), *n_matvec (may be NULL) the products it took.
 * Where this differs from the reference: the reference normalises every orthogonalised correction vector, also one that is zero or
 * rounding noise (start vectors that span an invariant subspace already: a diagonal matrix, a decoupled block, an exact eigenvector),
 * and never diagonalises the last vectors of a basis of min(n, 50 n_states) vectors when that is no multiple of n_states; it then
 * returns non-finite or wrong numbers.  Here the iteration ends on the basis it has when a correction is below 64 m 2^-53 of
 * max(its own norm in front of the m projections, 1), or when the basis holds n vectors; n_states == n is solved from the start
 * vectors alone.  A result reached in one of these ways, or through the reference's criterion on the correction vectors (their summed
 * squared norms below 1e-12), is returned only if every state's residual bears that criterion out,
 * |H x - e x|^2 <= 2e-12 (|H x|^2 + max diag^2); otherwise the call fails with SQMC_ERR_BREAKDOWN and a message, evals and evecs
 * undefined.  The iterates themselves are the reference's throughout. */
int sqmc_gpu_davidson(sqmc_spmv_plan *plan, const double *diag, int32_t n_states, const double *v0, double tol, double *evals, double *evecs, int32_t *n_matvec);
/* generate_sparse_ham_chem_upper_triangular (chemistry.f90:7639-8010) and the plan of the Davidson
 * matvec in one call, with the matrix never leaving the GPU: for a determinant list sorted by
 * (up,dn) the Hamiltonian is built and expanded to the full symmetric CSR on the device; diag[n]
 * (Davidson's preconditioner, more_tools.f90:2099-2110) and the number of stored upper-triangular
 * nonzeros come back.  Use the plan with sqmc_gpu_spmv_apply / _free. */
int sqmc_gpu_build_spmv_plan(sqmc_gpu_ctx *ctx, int64_t n, const uint64_t *up, const uint64_t *dn, sqmc_spmv_plan **plan, double *diag,
                             int64_t *out_nnz);
/* The principal submatrix of a resident plan as a plan of its own: dst(i, j) = src(sel[i], sel[j]).  sel[m]: row numbers of src,
 * 1-based like `indices`, strictly ascending.  The kept entries of a row stay in the source order, and sel ascends, so dst is entry
 * for entry the plan that sqmc_gpu_build_spmv_plan / sqmc_gpu_spmv_prepare build from the subset itself: its products and its
 * sqmc_gpu_davidson run return the same bits.  dst owns its buffers (sqmc_gpu_spmv_apply, sqmc_gpu_davidson, sqmc_gpu_spmv_free); src
 * is not modified and stays usable.  *out_nnz_full: the entries of dst's full CSR, (that number + m) / 2 of them in the stored triangle.
 * The preconditioner of dst is diag[sel] of src's.
 * SQMC_ERR_BAD_ARG: a null pointer, m < 1, m > n of src, sel out of range or not strictly ascending.  SQMC_ERR_UNSUPPORTED: the
 * measurement-only layout is on (SQMC_SPMV_UPPER_ATOMIC), whose stored triangle is not extracted.  A call that fails has written
 * neither *dst nor *out_nnz_full and holds no device memory. */
int sqmc_gpu_spmv_plan_submatrix(const sqmc_spmv_plan *src, int64_t m, const int64_t *sel, sqmc_spmv_plan **dst, int64_t *out_nnz_full);
/* shell_sort_real_rank1_int_rank1 without consider_sign (generic_sort.f90:685-735) on the host: a[n] by magnitude, greatest first,
 * iorder[n] carried along; not stable, so for equal magnitudes only this gives the reference's order.  Afterwards a changes sign as a
 * whole if a[0] < 0.  Touches no device. */
int sqmc_shell_sort_magnitude(int64_t n, double *a, int32_t *iorder);
int sqmc_gpu_spmv_sym_upper(int64_t n, const int64_t *row_counts, const int64_t *indices,
                            const double *values, const double *x, double *y);

/* replaces: hamiltonian_chem / hamiltonian_chem_time_sym through the dispatcher
 * semistoch.f90:2234-2302, for n (bra,ket) pairs; 0 where not connected. */
int sqmc_gpu_hamiltonian_batch(sqmc_gpu_ctx *ctx, int64_t n, const uint64_t *iu, const uint64_t *id,
                               const uint64_t *ju, const uint64_t *jd, double *h);

/* replaces: hamiltonian_chem (chemistry.f90:1260-1320) with the excitation level found from
 * the pair (no time-reversal symmetrisation even when time_sym is set); used to build
 * dtm_hb exactly as double_excitation_matrix_element_no_ref does (chemistry.f90:9615-9646). */
int sqmc_gpu_hamiltonian_chem_batch(sqmc_gpu_ctx *ctx, int64_t n, const uint64_t *iu, const uint64_t *id,
                                    const uint64_t *ju, const uint64_t *jd, double *h);

/* replaces: generate_sparse_ham_chem_upper_triangular (chemistry.f90:7639-8010) for a list
 * sorted by (up,dn): the symmetric Hamiltonian in the "upper triangular" storage above
 * (each row: its diagonal first, then columns j < i ascending; zero elements dropped).
 * Output arrays are allocated by the library; release each with sqmc_gpu_free. */
int sqmc_gpu_build_sparse_ham(sqmc_gpu_ctx *ctx, int64_t n, const uint64_t *up, const uint64_t *dn,
                              int64_t *out_nnz, int64_t **out_row_counts, int64_t **out_indices,
                              double **out_values);

/* test door onto the proposal kernel: off_diagonal_move_chem (chemistry.f90:4237-5084) for n
 * parents, child k of the batch drawing from rannyu state seeds[4k..4k+3]; returns det_j,
 * weight_j (= -tau*H/p) and the state after. */
int sqmc_gpu_propose_batch(sqmc_gpu_ctx *ctx, int64_t n, double tau, const uint64_t *up,
                           const uint64_t *dn, const int32_t *seeds, uint64_t *ju, uint64_t *jd,
                           double *weight_j, int32_t *seeds_after);

/* replaces: find_doubly_excited + find_important_connected_dets_chem + sort/dedup
 * (semistoch.f90:1750-2131, chemistry.f90:6819-7159, tools.f90:577-660) as used by
 * get_next_det_list (hci.f90:865) and generate_psi_t_connected_e_loc (semistoch.f90:27):
 * for n_ref reference dets with coefficients coeffs, the connections that pass the screen at eps/|c|, per class as the
 * reference has it: single excitations with |H| >= eps/|c| (chemistry.f90:6956, a tie is kept), chemistry doubles with
 * |H| > eps/|c| (chemistry.f90:7042, a tie is dropped; none when eps/|c| > max_double, :6995), HEG doubles with |H| > eps/|c|
 * (heg.f90:2608, 2629), the hops of hubbard2 (find_connected_dets_hubbard, hubbard.f90:5306-5457) and the connections of hubbardk
 * (find_connected_dets_hubbard_k, :5462) with |H c| > eps (the product itself is compared; a tie is dropped); H is the raw element,
 * before the time-reversal factors.  The reference det itself is included, except
 * that a det with c == 0 contributes nothing, its own slot included (the generator is not called for it, semistoch.f90:1762,
 * 1798, 1854, 1891).  Sorted by (up,dn), duplicates merged:
 * e_mix_num = sum_j H_ij c_j, e_mix_den = c_i on the reference determinants, else 0
 * (semistoch.f90:2039-2063).  diag_mode 0: the self slot carries H=0 (HCI, chemistry.f90:6896);
 * 1: it carries H_ii (find_connected_dets_chem, chemistry.f90:6574-6576, for C(T));
 * 2: "raw" -- no sort, no merge: every generated connection in generation order with
 *    e_mix_num = H_ki c_i and e_mix_den = i (0-based index of its reference determinant), what the
 *    weighted sums of second_order_pt_alias (hci.f90:1314-1660: term1, term2) are formed from.
 * out arrays are allocated by the library, release each with sqmc_gpu_free. */
int sqmc_gpu_hci_connections(sqmc_gpu_ctx *ctx, int64_t n_ref, const uint64_t *ref_up,
                             const uint64_t *ref_dn, const double *coeffs, double eps, int diag_mode,
                             int64_t *out_n, uint64_t **out_up, uint64_t **out_dn,
                             double **out_e_mix_num, double **out_e_mix_den);
/* The same restricted to slice `slice` of `n_slices` equal parts of the determinant-key range: every
 * connection belongs to exactly one slice and its merged sums are exact within it, so a PT stage whose
 * connected space does not fit one call (2^31 connections) is done slice by slice (the role of
 * n_energy_batch, hci.f90:642).  slice 0 of 1 = sqmc_gpu_hci_connections. */
int sqmc_gpu_hci_connections_slice(sqmc_gpu_ctx *ctx, int64_t n_ref, const uint64_t *ref_up, const uint64_t *ref_dn,
                                   const double *coeffs, double eps, int diag_mode, int32_t slice, int32_t n_slices, int64_t *out_n,
                                   uint64_t **out_up, uint64_t **out_dn, double **out_e_mix_num, double **out_e_mix_den);
/* replaces: the optional arguments core_up/dn, virt_up/dn, active_only of find_important_connected_dets_chem
 * (chemistry.f90:6840-6846, 6926-6947, 7087-7108) as get_next_det_list, second_order_pt and do_pt pass them down
 * (hci.f90:150-182, 386-389, 786-798, 914-920).  mode 0: no masks; 1: only determinants inside the active space (every core
 * orbital occupied, every virtual orbital empty); 2: only determinants outside it.  State of the context: applies to
 * sqmc_gpu_hci_connections(_slice) and sqmc_gpu_hci_pt2 until changed.  Chemistry only. */
int sqmc_gpu_hci_set_active_space(sqmc_gpu_ctx *ctx, uint64_t core_up, uint64_t core_dn, uint64_t virt_up, uint64_t virt_dn, int32_t mode);
/* replaces: get_new_diag_elem (chemistry.f90:9649-9739) and get_new_diag_elem_heg (heg.f90:3357-3453): H_aa of a determinant one
 * double excitation away from a determinant whose diagonal element is known, in O(n_elec) instead of O(n_elec^2).  Record i is
 * old_diag[i] = H of the source and pqrs[4i..4i+3] = p, q, r, s, the excitation p, q -> r, s in the reference's spin-orbital
 * numbering (1..norb up, norb+1..2 norb dn; r of p's spin, s of q's); new_up/new_dn[i] is the determinant it leads to.
 * form 0: one lane, the additions in the reference's statement order (bit for bit a left-to-right evaluation of them);
 * form 1: the two O(n) loops summed by a group of 16 lanes (the same terms, another order).
 * Every record is validated on the device before any table is read: orbitals in 1..2 norb, p != q, r != s, spins of p/r and q/s
 * equal, r and s occupied in the new determinant, p and q empty in it, electron numbers of the context.  One bad record makes
 * the call return SQMC_ERR_BAD_ARG with new_diag untouched.  chem and heg contexts; time_sym contexts (a determinant-basis
 * formula) and hubbard2 return SQMC_ERR_UNSUPPORTED.  For the electron gas the statements run with the integrals of
 * hamiltonian_heg (the reference's copy is never called and drops the kinetic part, see sqmc_amd/csrc/diag_update.h). */
int sqmc_gpu_diag_update_batch(sqmc_gpu_ctx *ctx, int64_t n, const double *old_diag, const int32_t *pqrs, const uint64_t *new_up,
                               const uint64_t *new_dn, int32_t form, double *new_diag);
/* replaces: the ref_diag_elems / diag_elems_info branch of find_doubly_excited (semistoch.f90:2182-2196), which second_order_pt
 * and second_order_pt_alias take.  mode 0 (default): H_aa of every connected determinant from scratch; 1: from the generator's
 * record by the O(N) update, one lane per determinant; 2: the same by 16-lane groups.  Single excitations and self slots are
 * recomputed from scratch in every mode, as the reference does (old_diag_elem = 1e51, chemistry.f90:6898, 6990).  State of the
 * context: honoured by sqmc_gpu_hci_pt2 (any slice count) and by a plan from sqmc_gpu_hci_pt2_stochastic_prepare (the mode as it
 * stands at prepare).  Modes 1 and 2 are refused (SQMC_ERR_UNSUPPORTED) on time_sym and hubbard2 contexts. */
int sqmc_gpu_hci_set_diag_update(sqmc_gpu_ctx *ctx, int32_t mode);
/* Test door, not for hosts: runs the bucket-boundary kernel of the short-list tail on the context's stream over caller-supplied
 * arrays.  keys: n0 >= 1 ascending 32-bit sort keys of a resident list (the door forms the key << 32 | index words).  B buckets;
 * every other input is B + 1 words or null: kb / hint (boundary keys of this step and about where they lie; kb null: no positions
 * are looked for, and pos must be null too), kb_prev / pos_prev (the boundaries scount was counted with and where they lay; either
 * null: equal numbers of residents), scount (spawns per bucket; needed with kb_out).  Outputs: pos (B + 1 words: first position
 * whose key is >= kb[j]), kb_out and hint_out (B words each: the next boundaries and their places; kb_out null: not made;
 * B <= 256 with kb_out). */
int sqmc_gpu_debug_bucket_boundaries(sqmc_gpu_ctx *ctx, int64_t n0, const uint32_t *keys, int32_t B, const uint32_t *kb, const uint32_t *hint,
                                     const uint32_t *kb_prev, const uint32_t *pos_prev, const uint32_t *scount, uint32_t *pos, uint32_t *kb_out,
                                     uint32_t *hint_out);
/* sqmc_gpu_hci_connections_slice with the record every connection carries for the update (diag_elems_info as
 * find_important_connected_dets_chem fills it, chemistry.f90:7148-7152): out_old_diag = H_ii of the source the connection was
 * generated from, out_pqrs = four int32 per connection, all 0 for a self slot or a single excitation.  Merged modes keep the record
 * of the first entry of each run of equal determinants in the sorted (stable: generation) order; the reference keeps whichever its
 * merge leaves, and any of them gives the same H_aa up to rounding.  The other outputs are those of the _slice entry bit for bit. */
int sqmc_gpu_hci_connections_record(sqmc_gpu_ctx *ctx, int64_t n_ref, const uint64_t *ref_up, const uint64_t *ref_dn, const double *coeffs,
                                    double eps, int diag_mode, int32_t slice, int32_t n_slices, int64_t *out_n, uint64_t **out_up,
                                    uint64_t **out_dn, double **out_e_mix_num, double **out_e_mix_den, double **out_old_diag,
                                    int32_t **out_pqrs);
/* replaces: second_order_pt (hci.f90:1100-1182), the deterministic Epstein-Nesbet correction of a variational wavefunction:
 * delta_e = sum_a (sum_i H_ai c_i)^2 / (E_var - H_aa) over the connected determinants outside the variational space, the inner
 * sum screened by |H_ai c_i| >= eps_pt; n_connections = connected determinants visited (the reference prints it).  Everything
 * stays on the device; n_slices > 1 does the connected space in parts of the determinant range.  Needs sqmc_gpu_set_hb_tables
 * (chem) like the generator; heg, hubbard2 and hubbardk (without space_sym) contexts need nothing more.  For a time-symmetrised wavefunction pass the determinant-basis expansion, as the reference does
 * (convert_time_symmetrized_to_dets, hci.f90:4365-4564) on a context initialised with time_sym = 0. */
int sqmc_gpu_hci_pt2(sqmc_gpu_ctx *ctx, int64_t n_var, const uint64_t *var_up, const uint64_t *var_dn, const double *coeffs, double e_var,
                     double eps_pt, int32_t n_slices, double *delta_e, int64_t *n_connections);
/* replaces: one sample of second_order_pt_alias (hci.f90:1314-1660), the semistochastic Epstein-Nesbet correction every HCI run uses
 * once the connected space no longer fits (the reference switches to it by itself, hci.f90:688-702).  The alias tables
 * (setup_alias, more_tools.f90:5603-5662), the 2 n_mc draws per sample of the serial rannyu stream (hci.f90:1438-1446), the merge of
 * repeats, Welford and the stopping rule stay in the caller; everything that scales with the connections is done here.
 *
 * prepare (hci.f90:1373-1436): uploads the variational wavefunction once -- determinants, coefficients, their sorted ranks -- and
 * owns the work buffers, which are reused from sample to sample and grow only when a sample has more raw connections than any before
 * it.  The list must be sorted by (up, dn) without repeats (hci.f90:1373-1380: an unsorted one is refused); n_mc >= 2.  Chemistry
 * (sqmc_gpu_set_hb_tables first) and HEG; the plan is not built for hubbard2 or hubbardk (refused).  p_i = |c_i| / sum |c|.
 * A context initialised with time_sym is refused (SQMC_ERR_UNSUPPORTED): on time-reversal representatives the estimator is biased
 * (two raw excitations of one source that reach one representative stay two connections, so term2 holds x'^2 + x''^2 where
 * (x' + x'')^2 is needed, and the eps_pt_big mask would see the element after the time-reversal factors).  Pass the
 * determinant-basis expansion on a context with time_sym = 0, as for sqmc_gpu_hci_pt2 and as the reference does.
 * The plan borrows ctx: free it before sqmc_gpu_finalize.  Active-space masks (sqmc_gpu_hci_set_active_space) are generator
 * state of ctx and apply to every sample as they stand when it runs. */
typedef struct sqmc_pt2s_plan sqmc_pt2s_plan;
int sqmc_gpu_hci_pt2_stochastic_prepare(sqmc_gpu_ctx *ctx, int64_t n_var, const uint64_t *var_up, const uint64_t *var_dn, const double *coeffs,
                                        double e_var, double eps_pt, double eps_pt_big, int32_t n_mc, sqmc_pt2s_plan **plan);
/* replaces: the body of the sample loop, hci.f90:1448-1640 (find_important_connected_dets of the sampled determinants, sort,
 * the term1 / term2 sums per connected determinant, binary_search against the variational list, H_kk, the sum).  ids: the n_distinct
 * distinct sampled determinants as 0-based positions in the variational list, ascending (what sort_and_merge_count_repeats,
 * tools.f90:1574-1602, leaves); counts: their multiplicities w_i >= 1.
 *   value = sum_k (term1^2 + term2 - term1_big^2 - term2_big) / (E_var - H_kk) / (n_mc (n_mc - 1))
 * over the connected determinants k outside the variational space, term1 = sum_i H_ki c_i w_i/p_i,
 * term2 = sum_i (H_ki c_i)^2 ((n_mc-1) w_i/p_i - (w_i/p_i)^2) over the connections the generator keeps at eps_pt, the _big sums over
 * those with |H_ki c_i| > eps_pt_big; n_connected = the number of those k.  The additions have one fixed order (generation order
 * within k, a fixed tree over k), so a sample returns the same bits run to run.  ids and counts go in, one double and one count
 * come back; nothing else crosses the bus.  A sample whose raw connection count reaches 2^31 is refused: this entry does not slice.
 * A refused sample leaves the plan usable.
 * The eps_pt_big test is strict for every excitation class, |H_ki c_i| > eps_pt_big (chemistry.f90:6978, 7139, heg.f90:2703).
 * A sampled determinant with c_i = 0 has p_i = 0 and w_i/p_i = inf; the generator emits nothing for it, its own slot included, so
 * nothing reads that value: the sample has the bits and the count of the same sample without it, and a sample of such
 * determinants only returns value = 0.0 and n_connected = 0. */
int sqmc_gpu_hci_pt2_stochastic_sample(sqmc_pt2s_plan *plan, int64_t n_distinct, const int64_t *ids, const int64_t *counts, double *value,
                                       int64_t *n_connected);
/* the plan's bookkeeping (any pointer may be NULL): n_alloc = how many times the per-connection buffers were (re)allocated, capacity =
 * connections they hold, last_raw = raw connections of the latest sample (before the merge; hci.f90:1452 n_connected_dets),
 * n_samples = samples evaluated */
int sqmc_gpu_hci_pt2_stochastic_stats(sqmc_pt2s_plan *plan, int64_t *n_alloc, int64_t *capacity, int64_t *last_raw, int64_t *n_samples);
/* replaces: the deallocations at the end of second_order_pt_alias (hci.f90:1642-1660) */
int sqmc_gpu_hci_pt2_stochastic_free(sqmc_pt2s_plan *plan);
/* replaces: get_1rdm (hci.f90:3198-3398), the one-body reduced density matrix of a variational wavefunction, spin-traced:
 *   rdm[p + norb r] = sum_sigma sum_i c_i c_k sign,   orbitals 0-based,
 * k = determinant i with the sigma electron moved p -> r (p occupied in i; r empty or r = p), sign = (-1)^(occupied sigma orbitals
 * strictly between p and r) = permutation_factor of the two sigma strings (tools.f90:1294-1396).  The diagonal is sum_i c_i^2 over
 * the determinants with p occupied, both spins added; the matrix is symmetric up to the order of its additions and its trace is
 * nelec sum c^2.  The list may come in any order: the library forms and sorts the determinant ranks itself (merge_sort2_up_dn at
 * :3328), and the result has the same bits for every order and from run to run (no floating-point atomics; a fixed tree).
 * A repeated determinant, a determinant with other electron numbers than the context's, or an orbital beyond norb: SQMC_ERR_BAD_ARG.
 * orbital_symmetries: norb labels (0..255) or NULL.  Given, pairs p, r of different label are skipped (:3351) and those entries are
 * exactly 0.0, the others the bits of the unfiltered call.  Every system type.  Contexts initialised with time_sym = 1 and hubbardk
 * with space_sym are refused (SQMC_ERR_UNSUPPORTED): pass the determinant-basis expansion (:3293-3308), the convention of
 * sqmc_gpu_hci_pt2.  A refused call leaves rdm untouched. */
int sqmc_gpu_hci_1rdm(sqmc_gpu_ctx *ctx, int64_t n_var, const uint64_t *var_up, const uint64_t *var_dn, const double *coeffs,
                      const int32_t *orbital_symmetries, double *rdm);
/* replaces: get_1rdm_with_pt (hci.f90:3400-3551): <0|rho|0> + <0|rho|1> + <1|rho|0>, |0> the variational wavefunction and |1> its
 * first-order correction.  The variational part is sqmc_gpu_hci_1rdm without a symmetry filter (:3483: the reference has none
 * there).  For every single excitation a of a variational determinant i that lies outside the variational space and inside the
 * connected space generated at eps_pt_big, sign c_i psi1_a is added to both rdm(p, r) and rdm(r, p);
 * psi1_a = (sum_j H_aj c_j) / (E_var - H_aa), the inner sum screened as the generator screens it (find_doubly_excited, :3471),
 * H_aa from scratch.  No <1|rho|1> term and no renormalisation: the trace stays nelec sum c^2.  The reference searches the
 * connected list first and the variational list second (:3488-3491); a variational determinant with c != 0 always occupies its own
 * slot of the connected list and one with c = 0 contributes nothing, so searching the variational list first gives the same matrix.
 * The connected space stays on the device (the generator of sqmc_gpu_hci_pt2); n_slices as there: every connected determinant
 * lives in one slice, so the slices' contributions add (in slice order).  n_connections = connected determinants visited.
 * The generator is handed the list in rank order, so the matrix has the same bits for every order of the caller's list.
 * Accepts the contexts sqmc_gpu_hci_pt2 accepts (chem after sqmc_gpu_set_hb_tables, heg, hubbard2, hubbardk without space_sym)
 * except that time_sym = 1 is refused as in sqmc_gpu_hci_1rdm.  Active-space masks (sqmc_gpu_hci_set_active_space) are generator
 * state of the context and apply as they stand.  Same bits run to run; a refused call leaves rdm and n_connections untouched. */
int sqmc_gpu_hci_1rdm_pt(sqmc_gpu_ctx *ctx, int64_t n_var, const uint64_t *var_up, const uint64_t *var_dn, const double *coeffs, double e_var,
                         double eps_pt_big, int32_t n_slices, double *rdm, int64_t *n_connections);
/* no counterpart in the reference (which stops at get_1rdm): the two-body reduced density matrix of a variational wavefunction
 * sum c_i |up_i, dn_i> in three spin blocks, each a dense norb^4 array with flat index p + norb (q + norb (r + norb s)), 0-based:
 *   rdm_aa = <a+_{p up} a+_{q up} a_{s up} a_{r up}>,  rdm_bb the same with dn,  rdm_ab = <a+_{p up} a+_{q dn} a_{s dn} a_{r up}>
 * with a determinant = all its up operators in front of all its dn operators (the ordering behind the library's Hamiltonian).
 * Nothing is renormalised: the traces sum_pq G[p,q,p,q] are 2 C(nup,2) sum c^2, 2 C(ndn,2) sum c^2 and nup ndn sum c^2.
 * blocks: 1 = aa, 2 = bb, 4 = ab, or-ed; the pointer of a block that is not requested is not read and may be NULL.
 * Evaluated through the (N-2)-electron intermediates K: every determinant emits one signed coefficient per pair of its electrons,
 * the records are sorted by (orbital pair, rank of K) and an entry is the product of two sorted columns.  No floating-point atomics
 * and a fixed order of additions: an entry has the same bits run to run, for every order of the caller's list and whichever other
 * blocks the call asked for; G[p,q,r,s] == G[r,s,p,q], G_aa[p,q,r,s] == -G_aa[q,p,r,s] == -G_aa[p,q,s,r] exactly, and every entry
 * no pair of determinants reaches is 0.0.  A block without a pair of electrons of its kind is all zeros.
 * Every system type; reads determinants and coefficients only.  SQMC_ERR_BAD_ARG: blocks outside 1..7, a requested block with a NULL
 * pointer, n_var < 1, a repeated determinant, a determinant with other electron numbers than the context's or an orbital beyond
 * norb.  SQMC_ERR_UNSUPPORTED: contexts with time_sym = 1 and hubbardk with space_sym (pass the determinant-basis expansion, as to
 * sqmc_gpu_hci_1rdm), a block whose intermediates need more than 64 key bits, a block of 2^32 - 1 records (n_var times the pairs of
 * electrons) or more.  A refused or failed call leaves all three arrays untouched. */
int sqmc_gpu_hci_2rdm(sqmc_gpu_ctx *ctx, int64_t n_var, const uint64_t *var_up, const uint64_t *var_dn, const double *coeffs,
                      int32_t blocks, double *rdm_aa, double *rdm_bb, double *rdm_ab);
/* no counterpart in the reference: the one-body transition density matrix of two coefficient vectors bra and ket over one
 * determinant list, spin-summed, in the index convention of sqmc_gpu_hci_1rdm:
 *   tdm[p + norb r] = <bra| a+_r a_p |ket> = sum_sigma sum_i sign ket_i bra_k,   orbitals 0-based,
 * k = determinant i with the sigma electron moved p -> r and sign as there; the diagonal is sum_i bra_i ket_i over the determinants
 * with p occupied, both spins added.  Nothing is renormalised: the trace is nelec <bra|ket>.  The block that owns (p, r), p < r,
 * forms both entries from one search of the sorted ranks (tdm[p,r] += sign ket_i bra_k, tdm[r,p] += sign bra_i ket_k), chunks of
 * the list in rank order are added in chunk order, up before dn, no floating-point atomics: an entry has the same bits run to run
 * and for every order of the caller's list; swapping bra and ket transposes the matrix exactly; with bra == ket, entries (p, r)
 * and (r, p) are both the bits of sqmc_gpu_hci_1rdm's entry (min, max).  orbital_symmetries: as in sqmc_gpu_hci_1rdm (filtered
 * entries exactly 0.0, the others the unfiltered bits).  Every system type.  Refusals and error codes are those of
 * sqmc_gpu_hci_1rdm (time_sym = 1, hubbardk with space_sym: SQMC_ERR_UNSUPPORTED; a repeated determinant, wrong electron numbers,
 * an orbital beyond norb, a label outside 0..255: SQMC_ERR_BAD_ARG).  A refused or failed call leaves tdm untouched. */
int sqmc_gpu_hci_1tdm(sqmc_gpu_ctx *ctx, int64_t n_var, const uint64_t *var_up, const uint64_t *var_dn, const double *bra, const double *ket,
                      const int32_t *orbital_symmetries, double *tdm);
/* no counterpart in the reference: the two-body transition density matrix of bra and ket over one determinant list, in the spin
 * blocks, index order and flat index of sqmc_gpu_hci_2rdm:
 *   tdm_aa = <bra| a+_{p up} a+_{q up} a_{s up} a_{r up} |ket>,  tdm_bb the same with dn,  tdm_ab = <bra| a+_{p up} a+_{q dn} a_{s dn} a_{r up} |ket>.
 * Nothing is renormalised.  The records, their sort and the owner scheme are the 2-RDM's; a record carries the signed bra and the
 * signed ket coefficient, and the owner of a pair of columns (A, B) keeps two sums for its one search, T[A,B] and T[B,A].  No
 * floating-point atomics and a fixed order of additions: the same bits run to run, for every order of the list and whichever other
 * blocks were asked for; T(bra, ket)[p,q,r,s] == T(ket, bra)[r,s,p,q] exactly; T(c, c) is the bytes of sqmc_gpu_hci_2rdm(c); the
 * antisymmetries of aa / bb under p <-> q and r <-> s hold exactly; every entry no pair of determinants reaches is 0.0 and nothing
 * is ever -0.0.  blocks, the refusals and the error codes are exactly those of sqmc_gpu_hci_2rdm.  A refused or failed call leaves
 * all three arrays untouched. */
int sqmc_gpu_hci_2tdm(sqmc_gpu_ctx *ctx, int64_t n_var, const uint64_t *var_up, const uint64_t *var_dn, const double *bra, const double *ket,
                      int32_t blocks, double *tdm_aa, double *tdm_bb, double *tdm_ab);
/* replaces: the integral rotation of generate_natorb_integrals (hci.f90:3683-3791): the context's one- and two-body integrals in
 * the orbitals  new_p = sum_k rot[k norb + p] old_k  (k, p 0-based, in the context's orbital order; row-major: the C-order memory of
 * the eigenvector matrix the 1-RDM is diagonalised into, the transpose of a column-major host's rdm(k, p)):
 *   (PQ|RS)' = sum_abcd U_aP U_bQ U_cR U_dS (ab|cd),   h'_PQ = sum_ab U_aP U_bQ h_ab,   E_nuc' = E_nuc,   U_kp = rot[k norb + p].
 * integrals_out: n_integrals + 1 doubles in the layout of sqmc_chem_cfg::integrals, addressed by the context's combine_2, so that a
 * new context can be initialised from it; every slot combine_2 does not address is 0.0.  The reference makes four passes over the
 * full norb^4 tensor; this makes two half transformations over orbital pairs and forms the packed (canonical) entries only, so the
 * result agrees with the reference's to rounding, not bit for bit.  rot may be any finite real matrix: orthogonality is not checked
 * (:3683-3791 does not check it either).  Same bits call to call (no atomics, a fixed summation order); a 0 or +-1 entry of rot
 * multiplies exactly, so the identity returns the input.  The context's own integrals stay as they are.
 * Chem contexts only, time_sym and n_core_orb do not matter: heg, hubbard2 and hubbardk return SQMC_ERR_UNSUPPORTED, as does a
 * combine_2 that is not a symmetric one-to-one pair index.  A null pointer or a non-finite entry of rot: SQMC_ERR_BAD_ARG.
 * A refused or failed call leaves integrals_out untouched.  Device memory: (norb (norb + 1) / 2)^2 doubles of work space. */
int sqmc_gpu_rotate_integrals(sqmc_gpu_ctx *ctx, const double *rot, double *integrals_out);
/* no counterpart in the reference (which stops at natural orbitals): the generalised Fock matrix, the orbital gradient and the
 * diagonal of the orbital Hessian of the fixed-coefficient energy, from the density matrices and the context's integrals.
 * Consumes: one_rdm = the spin-summed 1-RDM D[p,r] as sqmc_gpu_hci_1rdm writes it (norb^2 doubles, flat index p + norb r);
 * two_rdm_sf = the spin-free 2-RDM G = G_aa + G_bb + G_ab + G_ab[q,p,s,r] of the blocks of sqmc_gpu_hci_2rdm (norb^4 doubles, flat
 * index p + norb (q + norb (r + norb s))); h and (pr|qs) are the context's packed integrals.  Orbitals 0-based, in the context's
 * order; nothing is renormalised.  With E(U) = sum h'_pr D[p,r] + 1/2 sum (pr|qs)' G[p,q,r,s] on the integrals rotated as
 * sqmc_gpu_rotate_integrals rotates them and U(theta) = exp(theta (e_p e_q^T - e_q e_p^T)):
 *   fock[a + norb P]  = F[a,P] = sum_r h[a,r] D[P,r] + sum_qrs (ar|qs) G[P,q,r,s]
 *   grad[p + norb q]  = dE/dtheta at 0    = 2 (F[p,q] - F[q,p])
 *   hdiag[p + norb q] = d2E/dtheta2 at 0  = -2 (F[p,p] + F[q,q]) + Y[pq,pq] + Y[qp,qp] - 2 Y[pq,qp],  hdiag[p + norb p] = 0.0,
 *   Y[xP,yQ] = 2 h[x,y] D[P,Q] + 2 sum_rs { (xy|rs) G[P,r,Q,s] + (xr|ys) (G[P,Q,r,s] + G[P,s,r,Q]) }.
 * The formulas are evaluated literally for whatever arrays are passed; they are the derivatives when D is symmetric and
 * G[p,q,r,s] == G[r,s,p,q] == G[q,p,s,r], as the library's own matrices are.  Each output is norb^2 doubles; any may be NULL (it
 * is then not computed), not all three.  F is a blocked fp64 GEMM over (q,r,s) split over up to 512 blocks whose partial tiles a
 * second kernel adds in ascending order; vector FMAs, no floating-point atomics: the same bits call to call and whichever outputs
 * are asked for; grad[p,q] == -grad[q,p] and grad[p,p] == 0.0 exactly; no output holds -0.0.
 * Chem contexts only, time_sym and n_core_orb do not matter (only the integrals are read): heg, hubbard2 and hubbardk return
 * SQMC_ERR_UNSUPPORTED, as does a combine_2 sqmc_gpu_rotate_integrals refuses.  SQMC_ERR_BAD_ARG: a null context or input, all
 * outputs NULL, a non-finite entry of one_rdm or two_rdm_sf.  A refused or failed call leaves the outputs untouched.
 * Device memory: norb^4 doubles for G and up to 512 norb^2 for the partial tiles. */
int sqmc_gpu_orbital_gradient(sqmc_gpu_ctx *ctx, const double *one_rdm, const double *two_rdm_sf, double *fock_out, double *grad_out,
                              double *hdiag_out);
/* no counterpart in the reference: the one-index transformation of the context's integrals by a real norb x norb matrix kappa
 * (kappa[a norb + P] = kappa_aP, the layout of rot), the first-order coefficient in t of sqmc_gpu_rotate_integrals(I + t kappa):
 *   h~_PQ    = sum_a kappa_aP h_aQ + sum_b kappa_bQ h_Pb
 *   (PQ|RS)~ = sum_a kappa_aP (aQ|RS) + sum_b kappa_bQ (Pb|RS) + sum_c kappa_cR (PQ|cS) + sum_d kappa_dS (PQ|Rd),   E_nuc~ = 0.0
 * It keeps the 8-fold symmetry for any kappa.  integrals_out: n_integrals + 1 doubles in the layout of sqmc_chem_cfg::integrals,
 * addressed by the context's combine_2; the nuclear-energy slot and every slot combine_2 does not address are 0.0.  A half pass
 * over orbital pairs forms the first two terms (two fma chains in ascending index from 0.0, then added), a second pass adds the
 * half-transformed table to its transpose; one owner per entry, no floating-point atomics: the same bits call to call, exactly
 * linear under a scaling by a power of two, all +0.0 for kappa = 0.  Any finite real kappa (antisymmetry is not required here).
 * Chem contexts only: heg, hubbard2 and hubbardk return SQMC_ERR_UNSUPPORTED, as does a combine_2 sqmc_gpu_rotate_integrals
 * refuses.  A null pointer or a non-finite entry: SQMC_ERR_BAD_ARG.  A refused or failed call leaves integrals_out untouched.
 * Device memory: (norb (norb + 1) / 2)^2 doubles of work space. */
int sqmc_gpu_one_index_transform(sqmc_gpu_ctx *ctx, const double *kappa, double *integrals_out);
/* no counterpart in the reference: the resident plan of a second-order orbital step.  prepare makes the checks of
 * sqmc_gpu_orbital_gradient on the same two matrices, uploads them and the pair table once, computes F, the gradient and the
 * diagonal Hessian once and owns the work space of a Hessian-vector product (the partial tiles of the Fock GEMM, the work buffer
 * and the table of the one-index transformation, the transformed Fock matrix).  A refused or failed prepare leaves plan_out
 * untouched and holds nothing.  The plan borrows ctx: free it before sqmc_gpu_finalize. */
typedef struct sqmc_orbopt_plan sqmc_orbopt_plan;
int sqmc_gpu_orbopt_prepare(sqmc_gpu_ctx *ctx, const double *one_rdm, const double *two_rdm_sf, sqmc_orbopt_plan **plan_out);
/* what prepare computed, bit for bit what sqmc_gpu_orbital_gradient returns on the same inputs; any output may be NULL, not all */
int sqmc_gpu_orbopt_gradient(sqmc_orbopt_plan *plan, double *fock_out, double *grad_out, double *hdiag_out);
/* the orbital Hessian of the fixed-coefficient energy applied to an antisymmetric kappa (kappa[a norb + P] = kappa_aP):
 *   sigma[p + norb q] = d2/ds dt E(exp(s kappa + t (e_p e_q^T - e_q e_p^T))) at s = t = 0
 *                     = 2 (F~[p,q] - F~[q,p]) + 1/2 ((kappa g)[p,q] - (g kappa)[p,q]),
 * F~ the Fock formula of sqmc_gpu_orbital_gradient on the one-index-transformed table, g the gradient at kappa = 0; rotations as
 * sqmc_gpu_rotate_integrals'.  sigma(K_pq)[p,q] is hdiag[p,q].  norb^2 doubles go in and norb^2 come back.  Fixed order of
 * additions, no atomics: the same bits call to call and plan to plan; sigma[p,q] == -sigma[q,p], a 0.0 diagonal, no -0.0.
 * SQMC_ERR_BAD_ARG: a null argument, a non-finite entry, a kappa that is not exactly antisymmetric (kappa[p,q] != -kappa[q,p] or a
 * non-zero diagonal).  A refused or failed call leaves sigma_out untouched and the plan usable. */
int sqmc_gpu_orbopt_hessian_vector(sqmc_orbopt_plan *plan, const double *kappa, double *sigma_out);
int sqmc_gpu_orbopt_free(sqmc_orbopt_plan *plan);
/* replaces: get_zeroth_order_variational_greens_function (hci.f90:3849-4050) without its file output: the Green's function of a
 * variational wavefunction sum c_i |i> of energy e0 with the diagonal of H as the zeroth-order Hamiltonian of the N+-1 electron
 * spaces, spin-summed, at the frequencies w[0 .. n_w - 1]:
 *   g_np1[i_w + n_w (p + norb q)] = sum_sigma sum_i c_i c_k / (w - (H_mm - e0)),  m = i + q sigma (q empty in i), k = m - p sigma
 *   g_nm1[i_w + n_w (p + norb q)] = sum_sigma sum_i c_i c_k / (w - (e0 - H_mm)),  m = i - q sigma (q occupied in i), k = m + p sigma
 * orbitals 0-based, k in the list, H_mm = hamiltonian_chem of the N+-1 electron determinant m from scratch: the memory of the
 * reference's G0(n_w, norb, norb).  A term is the rounded product c_i c_k divided by the rounded denominator, as at :3944; only
 * the order of the additions differs from the reference's.  fermi_sign = 0: no fermionic sign, as the reference (:3944, :3963,
 * :3984, :4002).  fermi_sign = 1: the matrix elements <a_p (w - (H0 - E0))^-1 a+_q> and <a+_p (w - (E0 - H0))^-1 a_q> of its header
 * comment (:3859-3860): for p != q a term is multiplied by -(-1)^b (N+1) or (-1)^b (N-1), b = the sigma electrons strictly between
 * p and q; the diagonals, and the density of states sum_p g(w, p, p), are the same bits in both modes.
 * The list may be in any order and is sorted by rank here; no floating-point atomics and a fixed order of additions: the same bits
 * run to run, for every order of the caller's list, and for a frequency whatever other frequencies the call holds.
 * One of g_np1, g_nm1 may be NULL: that half is not computed.  A frequency on a pole gives what IEEE division gives.
 * SQMC_ERR_BAD_ARG: both outputs NULL, n_var <= 0, n_w <= 0, a non-finite e0 or w, fermi_sign not 0 or 1, a repeated determinant,
 * a determinant with other electron numbers than the context's or an orbital beyond norb.  SQMC_ERR_UNSUPPORTED: a context with
 * time_sym = 1 (pass the determinant-basis expansion, as to sqmc_gpu_hci_1rdm; :3895 stops there too) and every system other than
 * chem.  A refused call leaves the outputs untouched.  Work memory on the device does not grow with n_var * n_w. */
int sqmc_gpu_hci_greens_function(sqmc_gpu_ctx *ctx, int64_t n_var, const uint64_t *var_up, const uint64_t *var_dn,
                                 const double *coeffs, double e0, int32_t n_w, const double *w, int32_t fermi_sign,
                                 double *g_np1, double *g_nm1);
/* replaces: the off-diagonal histograms and weight ratios every walk of the reference keeps (off_diag_histograms = .true.,
 * do_walk.f90:104; gen_hist at 1420-1429; filled at 3619-3640 and in add_walker, 7603-7636; max_wt_ratio / min_wt_ratio at 3649-3661,
 * 7610-7622).  Context state, off by default: with it off a step launches exactly the kernels it launches without this entry.  On,
 * every step's spawn kernel also bins x = abs(weight_j)/tau = |H_ij| / p(i -> j) of each off-diagonal proposal with add_to_hist's
 * statements (more_tools.f90:5472-5495: 10001 unit-wide bins from 0, the last one open) and keeps the largest x per excitation
 * level and the smallest x over the proposals with x > 1e-9.  Walker lists and the 16 sums are bit-identical either way; steps run
 * un-pipelined while it is on, so the totals after N returned steps hold exactly the proposals of those N steps.
 * on != 0 allocates and zeroes at first use (64 sets of the counters, 20 MB: blocks add to different sets, get folds them); on = 0 keeps
 * the counts. */
int sqmc_gpu_set_spawn_diagnostics(sqmc_gpu_ctx *ctx, int32_t on);
/* zeroes counts, ratios and the NaN count (the reference does this once, before the run: do_walk.f90:1420-1429, 3432-3433) */
int sqmc_gpu_reset_spawn_diagnostics(sqmc_gpu_ctx *ctx);
/* replaces: the tables of do_walk.f90:3295-3311 and the ratios of 3313-3322, as data.  Waits for the context's streams.  Any pointer
 * may be NULL.  nbins = 10001; bins (any walker), bins_hf (proposals of iwalk == 1, slot 0 of the resident list), bins_single and
 * bins_double (chemistry only, proposals with weight_j != 0 by excitation_level, chemistry.f90:7162-7227): nbins counts each.
 * max_ratio_by_level[l]: largest x among proposals of excitation level l (count_excitations on both spin strings, the smaller of the
 * straight and the spin-swapped count with time_sym: 3654-3658; levels above 7 count as 7), -1e99 where none; max_ratio = the
 * largest of them, max_ratio_level = the lowest level that attains it (-1: none); min_ratio = 1e99 when nothing qualified (the
 * reference's initial values); n_nan = proposals whose x was a NaN (add_to_hist stops the run there: the caller should). */
int sqmc_gpu_get_spawn_diagnostics(sqmc_gpu_ctx *ctx, int32_t *nbins, int64_t *bins, int64_t *bins_hf, int64_t *bins_single,
                                   int64_t *bins_double, double max_ratio_by_level[8], double *max_ratio, int32_t *max_ratio_level,
                                   double *min_ratio, int64_t *n_nan);
void sqmc_gpu_free(void *p);

/* HIP-event timing on the library's streams.  level 0 off; 1 = only the longest kernel on the
 * critical path, on every 8th step (the annihilation kernel of a semistochastic walk, k_spawn of
 * a plain one: a timed launch cannot overlap its neighbours); 2 = every stage of every step.  get_timing returns the mean
 * milliseconds per step of each timer over the steps run since set_timing (n <= 32). */
int sqmc_gpu_set_timing(sqmc_gpu_ctx *ctx, int level);
int sqmc_gpu_get_timing(sqmc_gpu_ctx *ctx, int32_t *n, const char **names, float *ms);

#ifdef __cplusplus
}
#endif
#endif
