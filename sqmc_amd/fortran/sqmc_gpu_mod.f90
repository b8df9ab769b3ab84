!> sqmc_gpu_mod -- iso_c_binding view of include/sqmc_gpu.h for a Fortran host such as the
!> reference's do_walk.f90 / more_tools.f90 / hci.f90.  Every interface names the C entry point
!> it binds; INTEGRATION.md lists the reference call sites each one replaces.
!> Determinants cross the boundary as integer(c_int64_t) (the low word of the reference's
!> 128-bit ik, exactly as conv_128_to_64 does for MPI, mpi_routines.f90:671-680).
module sqmc_gpu_mod
  use iso_c_binding
  implicit none
  private
  public :: sqmc_chem_cfg, sqmc_heg_cfg, sqmc_gpu_init_heg, sqmc_hubbard_cfg, sqmc_gpu_init_hubbard, sqmc_hubbardk_cfg, sqmc_gpu_init_hubbardk, sqmc_step_params, sqmc_popctl, sqmc_gpu_run
  public :: sqmc_gpu_set_device, sqmc_gpu_init_chem, sqmc_gpu_finalize, sqmc_gpu_last_error, sqmc_gpu_set_hb_tables
  public :: sqmc_gpu_set_projector, sqmc_gpu_scale_projector, sqmc_gpu_set_ct_table, sqmc_gpu_upload_walkers
  public :: sqmc_gpu_num_walkers, sqmc_gpu_download_walkers, sqmc_gpu_step, sqmc_gpu_get_rng, sqmc_gpu_set_rng
  public :: sqmc_gpu_spmv_prepare, sqmc_gpu_spmv_apply, sqmc_gpu_spmv_free, sqmc_gpu_spmv_sym_upper
  public :: sqmc_gpu_hamiltonian_batch, sqmc_gpu_hamiltonian_chem_batch, sqmc_gpu_build_sparse_ham, sqmc_gpu_propose_batch
  public :: sqmc_gpu_hci_connections, sqmc_gpu_free, sqmc_gpu_set_timing, sqmc_gpu_get_timing
  public :: sqmc_gpu_det_owner, sqmc_gpu_shard_config, sqmc_gpu_shard_begin, sqmc_gpu_shard_pack, sqmc_gpu_shard_finish
  public :: sqmc_gpu_annihilate, sqmc_gpu_build_spmv_plan, sqmc_gpu_hci_connections_slice
  public :: sqmc_gpu_comm_unique_id, sqmc_gpu_comm_init, sqmc_gpu_comm_size, sqmc_gpu_set_owner_hash, sqmc_gpu_tail_stats, sqmc_gpu_last_tail, sqmc_gpu_slowest_steps, sqmc_gpu_set_chained_runs, sqmc_gpu_hci_pt2, sqmc_gpu_hci_set_active_space, sqmc_gpu_set_heatbath_tables, sqmc_gpu_propose_heatbath_batch, sqmc_heatbath_tables, sqmc_gpu_shard_step, sqmc_gpu_shard_run, sqmc_gpu_shard_time_split, sqmc_gpu_davidson
  public :: sqmc_gpu_set_hf_to_psit, sqmc_gpu_setup_efficient_heatbath, sqmc_gpu_get_heatbath_tables
  public :: sqmc_gpu_set_hf_to_psit_shard, sqmc_gpu_shard_finish_psit
  public :: sqmc_gpu_setup_cauchy_schwarz, sqmc_gpu_propose_cauchy_schwarz_batch
  public :: sqmc_gpu_diag_update_batch, sqmc_gpu_hci_set_diag_update, sqmc_gpu_hci_connections_record
  public :: sqmc_gpu_hci_pt2_stochastic_prepare, sqmc_gpu_hci_pt2_stochastic_sample, sqmc_gpu_hci_pt2_stochastic_stats, sqmc_gpu_hci_pt2_stochastic_free
  public :: sqmc_gpu_set_spawn_diagnostics, sqmc_gpu_reset_spawn_diagnostics, sqmc_gpu_get_spawn_diagnostics
  public :: sqmc_gpu_set_hubbardk_space_sym, sqmc_gpu_hubbardk_sym_images, sqmc_gpu_debug_bucket_boundaries
  public :: sqmc_gpu_hci_1rdm, sqmc_gpu_hci_1rdm_pt, sqmc_gpu_hci_2rdm, sqmc_gpu_hci_1tdm, sqmc_gpu_hci_2tdm, sqmc_gpu_rotate_integrals, sqmc_gpu_orbital_gradient, sqmc_gpu_hci_greens_function
  public :: sqmc_gpu_spmv_plan_submatrix, sqmc_shell_sort_magnitude
  public :: sqmc_gpu_one_index_transform, sqmc_gpu_orbopt_prepare, sqmc_gpu_orbopt_gradient, sqmc_gpu_orbopt_hessian_vector, sqmc_gpu_orbopt_free
  public :: sqmc_gpu_check

  integer(c_int), parameter, public :: SQMC_RNG_REPLAY = 0, SQMC_RNG_COUNTER = 1

  type, bind(C) :: sqmc_chem_cfg
    integer(c_int32_t) :: norb, nup, ndn, n_core_orb
    integer(c_int32_t) :: time_sym, z
    integer(c_int32_t) :: n_group
    type(c_ptr) :: product_table       ! int32 (0:8,0:8) stored [i*9+j]
    type(c_ptr) :: orbital_symmetries  ! int32 (0:norb)
    type(c_ptr) :: combine_2           ! int32 (0:norb+1,0:norb+1) stored [i*(norb+2)+j]
    integer(c_int64_t) :: n_integrals
    type(c_ptr) :: integrals           ! real(c_double) (0:n_integrals)
    integer(c_int32_t) :: rng_mode
    integer(c_int32_t) :: irand_seed(4)
    integer(c_int64_t) :: mwalk
  end type

  type, bind(C) :: sqmc_heg_cfg
    integer(c_int32_t) :: n_dim, norb, nup, ndn
    real(c_double) :: length_cell
    type(c_ptr) :: k_vectors           ! real(c_double) k_vectors(n_dim, norb), as in module heg
    integer(c_int32_t) :: rng_mode
    integer(c_int32_t) :: irand_seed(4)
    integer(c_int64_t) :: mwalk
  end type

  type, bind(C) :: sqmc_hubbard_cfg    ! hamiltonian_type 'hubbard2': the scalars of read_hubbard (walk, sqmc_gpu_hci_connections(_slice), sqmc_gpu_hci_pt2)
    integer(c_int32_t) :: l_x, l_y, pbc, nup, ndn
    real(c_double) :: t, U
    integer(c_int32_t) :: rng_mode
    integer(c_int32_t) :: irand_seed(4)
    integer(c_int64_t) :: mwalk
  end type

  type, bind(C) :: sqmc_hubbardk_cfg   ! hamiltonian_type 'hubbardk': the tables of generate_k_vectors (space_sym: sqmc_gpu_set_hubbardk_space_sym)
    integer(c_int32_t) :: l_x, l_y, nup, ndn
    real(c_double) :: t, U
    type(c_ptr) :: k_vectors           ! integer(c_int32_t) k_vectors(2, nsites), as in module hubbard
    type(c_ptr) :: k_energies          ! real(c_double) k_energies(nsites)
    integer(c_int32_t) :: rng_mode
    integer(c_int32_t) :: irand_seed(4)
    integer(c_int64_t) :: mwalk
  end type

  type, bind(C) :: sqmc_step_params
    real(c_double) :: tau, e_trial, reweight_factor_inv, r_initiator, min_wt, always_spawn_cutoff_wt
    integer(c_int32_t) :: initiator_power, initiator_min_distance, c_t_initiator, semistochastic, reached_w_abs_gen
    integer(c_int32_t) :: reserved
  end type

  ! the tables of setup_efficient_heatbath (chemistry.f90:1002-1225) as the reference holds them: c_loc of its module arrays
  type, bind(C) :: sqmc_heatbath_tables
    integer(c_int32_t) :: norb, reserved
    type(c_ptr) :: one_orbital_probabilities, two_orbital_probabilities
    type(c_ptr) :: three_orbital_probabilities_same_spin, three_orbital_probabilities_opposite_spin
    type(c_ptr) :: J_three_orbital_probabilities_same_spin, J_three_orbital_probabilities_opposite_spin
    type(c_ptr) :: q_three_orbital_probabilities_same_spin, q_three_orbital_probabilities_opposite_spin
    integer(c_int64_t) :: size_same, size_opposite
    type(c_ptr) :: four_orbital_probabilities_same_spin, four_orbital_probabilities_opposite_spin
    type(c_ptr) :: J_four_orbital_probabilities_same_spin, J_four_orbital_probabilities_opposite_spin
    type(c_ptr) :: q_four_orbital_probabilities_same_spin, q_four_orbital_probabilities_opposite_spin
    type(c_ptr) :: Htot_same, Htot_opposite
  end type

  type, bind(C) :: sqmc_popctl
    real(c_double) :: tau_sav, tau, tau_prev, e_trial, e_est, w_abs_gen_target, w_abs_gen
    real(c_double) :: r_initiator_sav, r_initiator, initiator_rescale_power, population_control_exponent
    real(c_double) :: reweight_factor_inv, reweight_factor_inv_max, e_num_cum, e_den_cum, min_wt, always_spawn_cutoff_wt
    integer(c_int32_t) :: reached_w_abs_gen, initiator_power, initiator_min_distance, c_t_initiator, semistochastic, reserved
    integer(c_int64_t) :: istep, n_equil
  end type

  interface
    integer(c_int) function sqmc_gpu_run(ctx, pc, nsteps, stats, totals) bind(C, name='sqmc_gpu_run')
      import; type(c_ptr), value :: ctx; type(sqmc_popctl), intent(inout) :: pc; integer(c_int64_t), value :: nsteps
      type(c_ptr), value :: stats; real(c_double), intent(out) :: totals(16)
    end function
    integer(c_int) function sqmc_gpu_build_spmv_plan(ctx, n, up, dn, plan, diag, out_nnz) bind(C, name='sqmc_gpu_build_spmv_plan')
      import; type(c_ptr), value :: ctx; integer(c_int64_t), value :: n; integer(c_int64_t), intent(in) :: up(*), dn(*)
      type(c_ptr), intent(out) :: plan; real(c_double), intent(out) :: diag(*); integer(c_int64_t), intent(out) :: out_nnz
    end function
    integer(c_int) function sqmc_gpu_annihilate(ctx, p, n_spawn, up, dn, wt, imp_distance, initiator, out_stats) bind(C, name='sqmc_gpu_annihilate')
      import; type(c_ptr), value :: ctx; type(sqmc_step_params), intent(in) :: p; integer(c_int64_t), value :: n_spawn
      integer(c_int64_t), intent(in) :: up(*), dn(*); real(c_double), intent(in) :: wt(*)
      integer(c_int8_t), intent(in) :: imp_distance(*), initiator(*); real(c_double), intent(out) :: out_stats(16)
    end function
    integer(c_int) function sqmc_gpu_comm_unique_id(id) bind(C, name='sqmc_gpu_comm_unique_id')
      import; integer(c_int8_t), intent(out) :: id(128)
    end function
    integer(c_int) function sqmc_gpu_comm_init(ctx, id) bind(C, name='sqmc_gpu_comm_init')
      import; type(c_ptr), value :: ctx; integer(c_int8_t), intent(in) :: id(128)
    end function
    integer(c_int) function sqmc_gpu_set_owner_hash(ctx, mode) bind(C, name='sqmc_gpu_set_owner_hash')
      import; type(c_ptr), value :: ctx; integer(c_int32_t), value :: mode
    end function
    integer(c_int) function sqmc_gpu_davidson(plan, diag, n_states, v0, tol, evals, evecs, n_matvec) bind(C, name='sqmc_gpu_davidson')
      import; type(c_ptr), value :: plan; real(c_double), intent(in) :: diag(*); integer(c_int32_t), value :: n_states
      type(c_ptr), value :: v0; real(c_double), value :: tol; real(c_double), intent(out) :: evals(*), evecs(*); integer(c_int32_t), intent(out) :: n_matvec
    end function
    integer(c_int) function sqmc_gpu_shard_time_split(ctx, us, steps, reset) bind(C, name='sqmc_gpu_shard_time_split')
      import; type(c_ptr), value :: ctx; real(c_double), intent(out) :: us(4); integer(c_int64_t), intent(out) :: steps; integer(c_int32_t), value :: reset
    end function
    integer(c_int) function sqmc_gpu_tail_stats(ctx, bucket_steps, bucket_retries) bind(C, name='sqmc_gpu_tail_stats')
      import; type(c_ptr), value :: ctx; integer(c_int64_t), intent(out) :: bucket_steps, bucket_retries
    end function
    integer(c_int) function sqmc_gpu_last_tail(ctx, info) bind(C, name='sqmc_gpu_last_tail')
      import; type(c_ptr), value :: ctx; integer(c_int32_t), intent(out) :: info(4)
    end function
    integer(c_int) function sqmc_gpu_set_chained_runs(ctx, on) bind(C, name='sqmc_gpu_set_chained_runs')
      import; type(c_ptr), value :: ctx; integer(c_int32_t), value :: on
    end function
    integer(c_int) function sqmc_gpu_slowest_steps(ctx, us, step) bind(C, name='sqmc_gpu_slowest_steps')
      import; type(c_ptr), value :: ctx; real(c_double), intent(out) :: us(4); integer(c_int64_t), intent(out) :: step(4)
    end function
    integer(c_int) function sqmc_gpu_hci_set_active_space(ctx, core_up, core_dn, virt_up, virt_dn, mode) bind(C, name='sqmc_gpu_hci_set_active_space')
      import; type(c_ptr), value :: ctx; integer(c_int64_t), value :: core_up, core_dn, virt_up, virt_dn; integer(c_int32_t), value :: mode
    end function
    ! get_new_diag_elem (chemistry.f90:9649-9739): H_aa from the source's H_ii and the excitation p, q -> r, s (pqrs(4, n), the
    ! reference's 1..2 norb numbering); form 0 one lane in the reference's order, 1 lane groups
    integer(c_int) function sqmc_gpu_diag_update_batch(ctx, n, old_diag, pqrs, new_up, new_dn, form, new_diag) bind(C, name='sqmc_gpu_diag_update_batch')
      import; type(c_ptr), value :: ctx; integer(c_int64_t), value :: n; real(c_double), intent(in) :: old_diag(*)
      integer(c_int32_t), intent(in) :: pqrs(*); integer(c_int64_t), intent(in) :: new_up(*), new_dn(*); integer(c_int32_t), value :: form
      real(c_double), intent(out) :: new_diag(*)
    end function
    ! off_diag_histograms (do_walk.f90:104, 3619-3661, 7603-7636): histograms of abs(weight_j)/tau and the max / min weight ratios.
    ! The arrays of get are optional on the C side: pass c_null_ptr for any that is not wanted.
    integer(c_int) function sqmc_gpu_set_spawn_diagnostics(ctx, on) bind(C, name='sqmc_gpu_set_spawn_diagnostics')
      import; type(c_ptr), value :: ctx; integer(c_int32_t), value :: on
    end function
    integer(c_int) function sqmc_gpu_reset_spawn_diagnostics(ctx) bind(C, name='sqmc_gpu_reset_spawn_diagnostics')
      import; type(c_ptr), value :: ctx
    end function
    integer(c_int) function sqmc_gpu_get_spawn_diagnostics(ctx, nbins, bins, bins_hf, bins_single, bins_double, max_ratio_by_level, max_ratio, &
        max_ratio_level, min_ratio, n_nan) bind(C, name='sqmc_gpu_get_spawn_diagnostics')
      import; type(c_ptr), value :: ctx; integer(c_int32_t), intent(out) :: nbins
      type(c_ptr), value :: bins, bins_hf, bins_single, bins_double      ! integer(c_int64_t)(10001) each, or c_null_ptr
      real(c_double), intent(out) :: max_ratio_by_level(8), max_ratio, min_ratio
      integer(c_int32_t), intent(out) :: max_ratio_level; integer(c_int64_t), intent(out) :: n_nan
    end function
    ! H_aa of the PT2 stages: 0 from scratch (default), 1 / 2 the O(N) update on one lane / by lane groups
    integer(c_int) function sqmc_gpu_hci_set_diag_update(ctx, mode) bind(C, name='sqmc_gpu_hci_set_diag_update')
      import; type(c_ptr), value :: ctx; integer(c_int32_t), value :: mode
    end function
    ! test door of the bucket-boundary kernel; every array but keys may be c_null_ptr (include/sqmc_gpu.h says which go together)
    integer(c_int) function sqmc_gpu_debug_bucket_boundaries(ctx, n0, keys, B, kb, hint, kb_prev, pos_prev, scount, pos, kb_out, hint_out) &
        bind(C, name='sqmc_gpu_debug_bucket_boundaries')
      import; type(c_ptr), value :: ctx; integer(c_int64_t), value :: n0; integer(c_int32_t), intent(in) :: keys(*); integer(c_int32_t), value :: B
      type(c_ptr), value :: kb, hint, kb_prev, pos_prev, scount, pos, kb_out, hint_out
    end function
    integer(c_int) function sqmc_gpu_hci_connections_record(ctx, n_ref, ref_up, ref_dn, coeffs, eps, diag_mode, slice, n_slices, out_n, out_up, out_dn, &
        out_num, out_den, out_old_diag, out_pqrs) bind(C, name='sqmc_gpu_hci_connections_record')
      import; type(c_ptr), value :: ctx; integer(c_int64_t), value :: n_ref; integer(c_int64_t), intent(in) :: ref_up(*), ref_dn(*)
      real(c_double), intent(in) :: coeffs(*); real(c_double), value :: eps; integer(c_int), value :: diag_mode
      integer(c_int32_t), value :: slice, n_slices
      integer(c_int64_t), intent(out) :: out_n; type(c_ptr), intent(out) :: out_up, out_dn, out_num, out_den, out_old_diag, out_pqrs
    end function
    integer(c_int) function sqmc_gpu_hci_pt2(ctx, n_var, var_up, var_dn, coeffs, e_var, eps_pt, n_slices, delta_e, n_connections) &
        bind(C, name='sqmc_gpu_hci_pt2')
      import; type(c_ptr), value :: ctx; integer(c_int64_t), value :: n_var; integer(c_int64_t), intent(in) :: var_up(*), var_dn(*)
      real(c_double), intent(in) :: coeffs(*); real(c_double), value :: e_var, eps_pt; integer(c_int32_t), value :: n_slices
      real(c_double), intent(out) :: delta_e; integer(c_int64_t), intent(out) :: n_connections
    end function
    ! get_1rdm (hci.f90:3198-3398): rdm(norb, norb) of a determinant list in any order; orbital_symmetries = c_loc of norb
    ! integer(c_int32_t) labels (pairs of different label are skipped, :3351) or c_null_ptr
    integer(c_int) function sqmc_gpu_hci_1rdm(ctx, n_var, var_up, var_dn, coeffs, orbital_symmetries, rdm) bind(C, name='sqmc_gpu_hci_1rdm')
      import; type(c_ptr), value :: ctx; integer(c_int64_t), value :: n_var; integer(c_int64_t), intent(in) :: var_up(*), var_dn(*)
      real(c_double), intent(in) :: coeffs(*); type(c_ptr), value :: orbital_symmetries; real(c_double), intent(out) :: rdm(*)
    end function
    ! get_1rdm_with_pt (hci.f90:3400-3551): <0|rho|0> + <0|rho|1> + <1|rho|0>, the connected space at eps_pt_big in n_slices parts
    integer(c_int) function sqmc_gpu_hci_1rdm_pt(ctx, n_var, var_up, var_dn, coeffs, e_var, eps_pt_big, n_slices, rdm, n_connections) &
        bind(C, name='sqmc_gpu_hci_1rdm_pt')
      import; type(c_ptr), value :: ctx; integer(c_int64_t), value :: n_var; integer(c_int64_t), intent(in) :: var_up(*), var_dn(*)
      real(c_double), intent(in) :: coeffs(*); real(c_double), value :: e_var, eps_pt_big; integer(c_int32_t), value :: n_slices
      real(c_double), intent(out) :: rdm(*); integer(c_int64_t), intent(out) :: n_connections
    end function
    ! the two-body reduced density matrix in spin blocks: rdm_aa, rdm_bb, rdm_ab = c_loc of arrays (norb, norb, norb, norb) indexed
    ! (p, q, r, s) = <a+_p a+_q a_s a_r>, or c_null_ptr for a block that is not requested; blocks = 1 (aa) + 2 (bb) + 4 (ab)
    integer(c_int) function sqmc_gpu_hci_2rdm(ctx, n_var, var_up, var_dn, coeffs, blocks, rdm_aa, rdm_bb, rdm_ab) bind(C, name='sqmc_gpu_hci_2rdm')
      import; type(c_ptr), value :: ctx; integer(c_int64_t), value :: n_var; integer(c_int64_t), intent(in) :: var_up(*), var_dn(*)
      real(c_double), intent(in) :: coeffs(*); integer(c_int32_t), value :: blocks; type(c_ptr), value :: rdm_aa, rdm_bb, rdm_ab
    end function
    ! the one-body transition density matrix tdm(norb, norb) of two vectors over one list, tdm(p, r) = <bra| a+_r a_p |ket> spin-summed;
    ! orbital_symmetries as in sqmc_gpu_hci_1rdm
    integer(c_int) function sqmc_gpu_hci_1tdm(ctx, n_var, var_up, var_dn, bra, ket, orbital_symmetries, tdm) bind(C, name='sqmc_gpu_hci_1tdm')
      import; type(c_ptr), value :: ctx; integer(c_int64_t), value :: n_var; integer(c_int64_t), intent(in) :: var_up(*), var_dn(*)
      real(c_double), intent(in) :: bra(*), ket(*); type(c_ptr), value :: orbital_symmetries; real(c_double), intent(out) :: tdm(*)
    end function
    ! the two-body transition density matrix in the spin blocks of sqmc_gpu_hci_2rdm: (p, q, r, s) = <bra| a+_p a+_q a_s a_r |ket>
    integer(c_int) function sqmc_gpu_hci_2tdm(ctx, n_var, var_up, var_dn, bra, ket, blocks, tdm_aa, tdm_bb, tdm_ab) bind(C, name='sqmc_gpu_hci_2tdm')
      import; type(c_ptr), value :: ctx; integer(c_int64_t), value :: n_var; integer(c_int64_t), intent(in) :: var_up(*), var_dn(*)
      real(c_double), intent(in) :: bra(*), ket(*); integer(c_int32_t), value :: blocks; type(c_ptr), value :: tdm_aa, tdm_bb, tdm_ab
    end function
    ! the integral rotation of generate_natorb_integrals (hci.f90:3683-3791): rot(norb, norb) with rot(p, k) = component on the
    ! context's orbital k of new orbital p (column-major; the C side reads rot[k norb + p], 0-based); integrals_out(0:n_integrals)
    ! in the layout of sqmc_chem_cfg%integrals.  Chem contexts only
    integer(c_int) function sqmc_gpu_rotate_integrals(ctx, rot, integrals_out) bind(C, name='sqmc_gpu_rotate_integrals')
      import; type(c_ptr), value :: ctx; real(c_double), intent(in) :: rot(*); real(c_double), intent(out) :: integrals_out(*)
    end function
    ! the generalised Fock matrix, the orbital gradient and the diagonal orbital Hessian from one_rdm(norb, norb) (as sqmc_gpu_hci_1rdm
    ! writes it) and the spin-free two_rdm_sf(norb, norb, norb, norb); fock_out, grad_out, hdiag_out = c_loc of arrays (norb, norb)
    ! indexed (a, P) / (p, q), or c_null_ptr for one that is not wanted (not all three).  Chem contexts only
    integer(c_int) function sqmc_gpu_orbital_gradient(ctx, one_rdm, two_rdm_sf, fock_out, grad_out, hdiag_out) bind(C, name='sqmc_gpu_orbital_gradient')
      import; type(c_ptr), value :: ctx; real(c_double), intent(in) :: one_rdm(*), two_rdm_sf(*); type(c_ptr), value :: fock_out, grad_out, hdiag_out
    end function
    ! the one-index transformation of the integrals by kappa(norb, norb), the first-order coefficient of sqmc_gpu_rotate_integrals
    ! (identity + t kappa); the C side reads kappa[a norb + P] = kappa_aP, the layout of rot; integrals_out(0:n_integrals).  Chem contexts only
    integer(c_int) function sqmc_gpu_one_index_transform(ctx, kappa, integrals_out) bind(C, name='sqmc_gpu_one_index_transform')
      import; type(c_ptr), value :: ctx; real(c_double), intent(in) :: kappa(*); real(c_double), intent(out) :: integrals_out(*)
    end function
    ! the resident plan of a second-order orbital step: the matrices of sqmc_gpu_orbital_gradient uploaded once; F, the gradient and
    ! the diagonal Hessian computed once.  The plan borrows ctx: free it before sqmc_gpu_finalize
    integer(c_int) function sqmc_gpu_orbopt_prepare(ctx, one_rdm, two_rdm_sf, plan_out) bind(C, name='sqmc_gpu_orbopt_prepare')
      import; type(c_ptr), value :: ctx; real(c_double), intent(in) :: one_rdm(*), two_rdm_sf(*); type(c_ptr), intent(out) :: plan_out
    end function
    integer(c_int) function sqmc_gpu_orbopt_gradient(plan, fock_out, grad_out, hdiag_out) bind(C, name='sqmc_gpu_orbopt_gradient')
      import; type(c_ptr), value :: plan, fock_out, grad_out, hdiag_out
    end function
    ! sigma(norb, norb) indexed (p, q) = the orbital Hessian applied to the antisymmetric kappa (the C side reads kappa[a norb + P])
    integer(c_int) function sqmc_gpu_orbopt_hessian_vector(plan, kappa, sigma_out) bind(C, name='sqmc_gpu_orbopt_hessian_vector')
      import; type(c_ptr), value :: plan; real(c_double), intent(in) :: kappa(*); real(c_double), intent(out) :: sigma_out(*)
    end function
    integer(c_int) function sqmc_gpu_orbopt_free(plan) bind(C, name='sqmc_gpu_orbopt_free')
      import; type(c_ptr), value :: plan
    end function
    ! get_zeroth_order_variational_greens_function (hci.f90:3849-4050) without its files: g_np1(n_w, norb, norb) and
    ! g_nm1(n_w, norb, norb) = c_loc of the arrays, or c_null_ptr for a half that is not wanted; fermi_sign = 0 is the reference
    integer(c_int) function sqmc_gpu_hci_greens_function(ctx, n_var, var_up, var_dn, coeffs, e0, n_w, w, fermi_sign, g_np1, g_nm1) &
        bind(C, name='sqmc_gpu_hci_greens_function')
      import; type(c_ptr), value :: ctx; integer(c_int64_t), value :: n_var; integer(c_int64_t), intent(in) :: var_up(*), var_dn(*)
      real(c_double), intent(in) :: coeffs(*); real(c_double), value :: e0; integer(c_int32_t), value :: n_w
      real(c_double), intent(in) :: w(*); integer(c_int32_t), value :: fermi_sign; type(c_ptr), value :: g_np1, g_nm1
    end function
    ! second_order_pt_alias (hci.f90:1314-1660): the variational wavefunction and the work buffers stay on the device (prepare),
    ! one call per sample with the merged draws (0-based ids, ascending, and their counts), free at the end; chem and heg contexts
    ! (hubbard2 and hubbardk are refused)
    integer(c_int) function sqmc_gpu_hci_pt2_stochastic_prepare(ctx, n_var, var_up, var_dn, coeffs, e_var, eps_pt, eps_pt_big, n_mc, plan) &
        bind(C, name='sqmc_gpu_hci_pt2_stochastic_prepare')
      import; type(c_ptr), value :: ctx; integer(c_int64_t), value :: n_var; integer(c_int64_t), intent(in) :: var_up(*), var_dn(*)
      real(c_double), intent(in) :: coeffs(*); real(c_double), value :: e_var, eps_pt, eps_pt_big; integer(c_int32_t), value :: n_mc
      type(c_ptr), intent(out) :: plan
    end function
    integer(c_int) function sqmc_gpu_hci_pt2_stochastic_sample(plan, n_distinct, ids, counts, value, n_connected) &
        bind(C, name='sqmc_gpu_hci_pt2_stochastic_sample')
      import; type(c_ptr), value :: plan; integer(c_int64_t), value :: n_distinct; integer(c_int64_t), intent(in) :: ids(*), counts(*)
      real(c_double), intent(out) :: value; integer(c_int64_t), intent(out) :: n_connected
    end function
    integer(c_int) function sqmc_gpu_hci_pt2_stochastic_stats(plan, n_alloc, capacity, last_raw, n_samples) &
        bind(C, name='sqmc_gpu_hci_pt2_stochastic_stats')
      import; type(c_ptr), value :: plan; integer(c_int64_t), intent(out) :: n_alloc, capacity, last_raw, n_samples
    end function
    integer(c_int) function sqmc_gpu_hci_pt2_stochastic_free(plan) bind(C, name='sqmc_gpu_hci_pt2_stochastic_free')
      import; type(c_ptr), value :: plan
    end function
    integer(c_int) function sqmc_gpu_set_heatbath_tables(ctx, t) bind(C, name='sqmc_gpu_set_heatbath_tables')
      import; type(c_ptr), value :: ctx; type(sqmc_heatbath_tables), intent(in) :: t
    end function
    ! setup_efficient_heatbath (chemistry.f90:1002-1225) + check_heatbath_unbiased (9330-9375) done by the library; the tables it built
    integer(c_int) function sqmc_gpu_setup_efficient_heatbath(ctx, is_heatbath_unbiased) bind(C, name='sqmc_gpu_setup_efficient_heatbath')
      import; type(c_ptr), value :: ctx; integer(c_int32_t), intent(out) :: is_heatbath_unbiased
    end function
    integer(c_int) function sqmc_gpu_get_heatbath_tables(ctx, t, n_orb_uniq_sym) bind(C, name='sqmc_gpu_get_heatbath_tables')
      import; type(c_ptr), value :: ctx; type(sqmc_heatbath_tables), intent(out) :: t; integer(c_int32_t), intent(out) :: n_orb_uniq_sym
    end function
    integer(c_int) function sqmc_gpu_propose_heatbath_batch(ctx, n, tau, up, dn, seeds, det_j_up, det_j_dn, weight_j, seeds_after) &
        bind(C, name='sqmc_gpu_propose_heatbath_batch')
      import; type(c_ptr), value :: ctx; integer(c_int64_t), value :: n; real(c_double), value :: tau
      integer(c_int64_t), intent(in) :: up(*), dn(*); integer(c_int32_t), intent(in) :: seeds(*)
      integer(c_int64_t), intent(out) :: det_j_up(*), det_j_dn(*); real(c_double), intent(out) :: weight_j(*); integer(c_int32_t), intent(out) :: seeds_after(*)
    end function
    ! proposal_method 'CauchySchwarz': setup_orb_by_symm's tables (chemistry.f90:2505-2523), before any H-dependent state
    integer(c_int) function sqmc_gpu_setup_cauchy_schwarz(ctx, n_clamped) bind(C, name='sqmc_gpu_setup_cauchy_schwarz')
      import; type(c_ptr), value :: ctx; integer(c_int32_t), intent(out) :: n_clamped
    end function
    integer(c_int) function sqmc_gpu_propose_cauchy_schwarz_batch(ctx, n, tau, up, dn, seeds, det_j_up, det_j_dn, weight_j, seeds_after) &
        bind(C, name='sqmc_gpu_propose_cauchy_schwarz_batch')
      import; type(c_ptr), value :: ctx; integer(c_int64_t), value :: n; real(c_double), value :: tau
      integer(c_int64_t), intent(in) :: up(*), dn(*); integer(c_int32_t), intent(in) :: seeds(*)
      integer(c_int64_t), intent(out) :: det_j_up(*), det_j_dn(*); real(c_double), intent(out) :: weight_j(*); integer(c_int32_t), intent(out) :: seeds_after(*)
    end function
    integer(c_int) function sqmc_gpu_comm_size(ctx, nranks) bind(C, name='sqmc_gpu_comm_size')
      import; type(c_ptr), value :: ctx; integer(c_int32_t), intent(out) :: nranks
    end function
    integer(c_int) function sqmc_gpu_shard_step(ctx, p, out_stats) bind(C, name='sqmc_gpu_shard_step')
      import; type(c_ptr), value :: ctx; type(sqmc_step_params), intent(in) :: p; real(c_double), intent(out) :: out_stats(16)
    end function
    integer(c_int) function sqmc_gpu_shard_run(ctx, pc, nsteps, stats, totals) bind(C, name='sqmc_gpu_shard_run')
      import; type(c_ptr), value :: ctx; type(sqmc_popctl), intent(inout) :: pc; integer(c_int64_t), value :: nsteps
      type(c_ptr), value :: stats; real(c_double), intent(out) :: totals(16)
    end function
    integer(c_int) function sqmc_gpu_det_owner(ctx, n, up, dn, nranks, owner) bind(C, name='sqmc_gpu_det_owner')
      import; type(c_ptr), value :: ctx; integer(c_int64_t), value :: n; integer(c_int64_t), intent(in) :: up(*), dn(*)
      integer(c_int32_t), value :: nranks; integer(c_int32_t), intent(out) :: owner(*)
    end function
    integer(c_int) function sqmc_gpu_shard_config(ctx, rank, nranks, n_imp_local, global_row) bind(C, name='sqmc_gpu_shard_config')
      import; type(c_ptr), value :: ctx; integer(c_int32_t), value :: rank, nranks; integer(c_int64_t), value :: n_imp_local
      integer(c_int32_t), intent(in) :: global_row(*)
    end function
    integer(c_int) function sqmc_gpu_shard_begin(ctx, p, x_global_dev, n_children) bind(C, name='sqmc_gpu_shard_begin')
      import; type(c_ptr), value :: ctx; type(sqmc_step_params), intent(in) :: p; type(c_ptr), value :: x_global_dev
      integer(c_int64_t), intent(out) :: n_children
    end function
    integer(c_int) function sqmc_gpu_shard_pack(ctx, p, x_global_dev, send_dev, cap_records, send_counts) bind(C, name='sqmc_gpu_shard_pack')
      import; type(c_ptr), value :: ctx; type(sqmc_step_params), intent(in) :: p; type(c_ptr), value :: x_global_dev, send_dev
      integer(c_int64_t), value :: cap_records; integer(c_int64_t), intent(out) :: send_counts(*)
    end function
    integer(c_int) function sqmc_gpu_shard_finish(ctx, p, recv_dev, n_recv, out_stats) bind(C, name='sqmc_gpu_shard_finish')
      import; type(c_ptr), value :: ctx; type(sqmc_step_params), intent(in) :: p; type(c_ptr), value :: recv_dev
      integer(c_int64_t), value :: n_recv; real(c_double), intent(out) :: out_stats(16)
    end function
    integer(c_int) function sqmc_gpu_set_device(device) bind(C, name='sqmc_gpu_set_device')
      import; integer(c_int), value :: device
    end function
    integer(c_int) function sqmc_gpu_init_chem(cfg, ctx) bind(C, name='sqmc_gpu_init_chem')
      import; type(sqmc_chem_cfg), intent(in) :: cfg; type(c_ptr), intent(out) :: ctx
    end function
    integer(c_int) function sqmc_gpu_init_heg(cfg, ctx) bind(C, name='sqmc_gpu_init_heg')
      import; type(sqmc_heg_cfg), intent(in) :: cfg; type(c_ptr), intent(out) :: ctx
    end function
    integer(c_int) function sqmc_gpu_init_hubbard(cfg, ctx) bind(C, name='sqmc_gpu_init_hubbard')
      import; type(sqmc_hubbard_cfg), intent(in) :: cfg; type(c_ptr), intent(out) :: ctx
    end function
    integer(c_int) function sqmc_gpu_init_hubbardk(cfg, ctx) bind(C, name='sqmc_gpu_init_hubbardk')
      import; type(sqmc_hubbardk_cfg), intent(in) :: cfg; type(c_ptr), intent(out) :: ctx
    end function
    ! space_sym = .true. for hubbardk: z, p and the module variables c4_map(3, nsites), reflection_map(nsites) of hubbard.f90 as they are
    integer(c_int) function sqmc_gpu_set_hubbardk_space_sym(ctx, z, p, c4_map, reflection_map) bind(C, name='sqmc_gpu_set_hubbardk_space_sym')
      import; type(c_ptr), value :: ctx; integer(c_int32_t), value :: z, p; integer(c_int32_t), intent(in) :: c4_map(3, *), reflection_map(*)
    end function
    ! generate_fourfold_k_configs_efficient for a list: images and phases as (16, n) arrays
    integer(c_int) function sqmc_gpu_hubbardk_sym_images(ctx, n, up, dn, images_up, images_dn, phases, rep_up, rep_dn, phase_w_rep, norm, num_distinct) &
        bind(C, name='sqmc_gpu_hubbardk_sym_images')
      import; type(c_ptr), value :: ctx; integer(c_int64_t), value :: n; integer(c_int64_t), intent(in) :: up(*), dn(*)
      integer(c_int64_t), intent(out) :: images_up(16, *), images_dn(16, *), rep_up(*), rep_dn(*)
      integer(c_int32_t), intent(out) :: phases(16, *), phase_w_rep(*), num_distinct(*); real(c_double), intent(out) :: norm(*)
    end function
    integer(c_int) function sqmc_gpu_finalize(ctx) bind(C, name='sqmc_gpu_finalize')
      import; type(c_ptr), value :: ctx
    end function
    type(c_ptr) function sqmc_gpu_last_error() bind(C, name='sqmc_gpu_last_error')
      import
    end function
    integer(c_int) function sqmc_gpu_set_hb_tables(ctx, n_hb, hb_r, hb_s, hb_absH, n_pq, pq_ind, pq_count, max_double) &
        bind(C, name='sqmc_gpu_set_hb_tables')
      import; type(c_ptr), value :: ctx; integer(c_int64_t), value :: n_hb; integer(c_int32_t), intent(in) :: hb_r(*), hb_s(*)
      real(c_double), intent(in) :: hb_absH(*); integer(c_int32_t), value :: n_pq; integer(c_int64_t), intent(in) :: pq_ind(*)
      integer(c_int32_t), intent(in) :: pq_count(*); real(c_double), value :: max_double
    end function
    integer(c_int) function sqmc_gpu_set_projector(ctx, n_imp, nnz, row_counts, indices, values) bind(C, name='sqmc_gpu_set_projector')
      import; type(c_ptr), value :: ctx; integer(c_int64_t), value :: n_imp, nnz
      integer(c_int64_t), intent(in) :: row_counts(*), indices(*); real(c_double), intent(in) :: values(*)
    end function
    integer(c_int) function sqmc_gpu_scale_projector(ctx, ratio) bind(C, name='sqmc_gpu_scale_projector')
      import; type(c_ptr), value :: ctx; real(c_double), value :: ratio
    end function
    integer(c_int) function sqmc_gpu_set_ct_table(ctx, n, up, dn, e_num, e_den) bind(C, name='sqmc_gpu_set_ct_table')
      import; type(c_ptr), value :: ctx; integer(c_int64_t), value :: n; integer(c_int64_t), intent(in) :: up(*), dn(*)
      real(c_double), intent(in) :: e_num(*), e_den(*)
    end function
    ! hf_to_psit = .true. (do_walk.f90:378): psit_ct_index = my_locations_of_psit (1849-1886), cdet_psi_t in label order (1258), diag_elems (1091-1116)
    integer(c_int) function sqmc_gpu_set_hf_to_psit(ctx, n_psit, psit_ct_index, cdet_psi_t, diag_elems, sum_order) bind(C, name='sqmc_gpu_set_hf_to_psit')
      import; type(c_ptr), value :: ctx; integer(c_int64_t), value :: n_psit; integer(c_int64_t), intent(in) :: psit_ct_index(*)
      real(c_double), intent(in) :: cdet_psi_t(*), diag_elems(*); integer(c_int32_t), value :: sum_order
    end function
    ! hf_to_psit on a sharded walk (do_walk.f90:1808-1886): this rank's C(T) share and Psi_T entries, after sqmc_gpu_shard_config
    integer(c_int) function sqmc_gpu_set_hf_to_psit_shard(ctx, n_ct_local, ct_index, diag_elems, n_psit_local, psit_slot, psit_mask, &
                                                         n_psit, cdet_psi_t, sum_order) bind(C, name='sqmc_gpu_set_hf_to_psit_shard')
      import; type(c_ptr), value :: ctx; integer(c_int64_t), value :: n_ct_local, n_psit_local, n_psit
      integer(c_int64_t), intent(in) :: ct_index(*), psit_slot(*), psit_mask(*)
      real(c_double), intent(in) :: diag_elems(*), cdet_psi_t(*); integer(c_int32_t), value :: sum_order
    end function
    ! shard_finish of a sharded hf_to_psit step without a communicator: allreduce is an integer(c_int) function(buf_dev, n, user)
    ! bind(C) that sums the n doubles at buf_dev over ranks in place (e.g. MPI_Allreduce through a host copy), passed as c_funloc
    integer(c_int) function sqmc_gpu_shard_finish_psit(ctx, p, recv_dev, n_recv, reduce_buf_dev, allreduce, user, out_stats) &
        bind(C, name='sqmc_gpu_shard_finish_psit')
      import; type(c_ptr), value :: ctx; type(sqmc_step_params), intent(in) :: p; type(c_ptr), value :: recv_dev
      integer(c_int64_t), value :: n_recv; type(c_ptr), value :: reduce_buf_dev; type(c_funptr), value :: allreduce
      type(c_ptr), value :: user; real(c_double), intent(out) :: out_stats(16)
    end function
    integer(c_int) function sqmc_gpu_upload_walkers(ctx, n, up, dn, wt, imp_distance, initiator, perm_sign, matrix_elements, e_num, e_den) &
        bind(C, name='sqmc_gpu_upload_walkers')
      import; type(c_ptr), value :: ctx; integer(c_int64_t), value :: n; integer(c_int64_t), intent(in) :: up(*), dn(*)
      real(c_double), intent(in) :: wt(*), matrix_elements(*), e_num(*), e_den(*)
      integer(c_int8_t), intent(in) :: imp_distance(*), initiator(*), perm_sign(*)
    end function
    integer(c_int) function sqmc_gpu_num_walkers(ctx, n) bind(C, name='sqmc_gpu_num_walkers')
      import; type(c_ptr), value :: ctx; integer(c_int64_t), intent(out) :: n
    end function
    integer(c_int) function sqmc_gpu_download_walkers(ctx, cap, n, up, dn, wt, imp_distance, initiator, matrix_elements, e_num, e_den) &
        bind(C, name='sqmc_gpu_download_walkers')
      import; type(c_ptr), value :: ctx; integer(c_int64_t), value :: cap; integer(c_int64_t), intent(out) :: n
      integer(c_int64_t), intent(out) :: up(*), dn(*); real(c_double), intent(out) :: wt(*), matrix_elements(*), e_num(*), e_den(*)
      integer(c_int8_t), intent(out) :: imp_distance(*), initiator(*)
    end function
    integer(c_int) function sqmc_gpu_step(ctx, p, out_stats) bind(C, name='sqmc_gpu_step')
      import; type(c_ptr), value :: ctx; type(sqmc_step_params), intent(in) :: p; real(c_double), intent(out) :: out_stats(16)
    end function
    integer(c_int) function sqmc_gpu_get_rng(ctx, seed) bind(C, name='sqmc_gpu_get_rng')
      import; type(c_ptr), value :: ctx; integer(c_int32_t), intent(out) :: seed(4)
    end function
    integer(c_int) function sqmc_gpu_set_rng(ctx, seed) bind(C, name='sqmc_gpu_set_rng')
      import; type(c_ptr), value :: ctx; integer(c_int32_t), intent(in) :: seed(4)
    end function
    integer(c_int) function sqmc_gpu_spmv_prepare(n, row_counts, indices, values, plan) bind(C, name='sqmc_gpu_spmv_prepare')
      import; integer(c_int64_t), value :: n; integer(c_int64_t), intent(in) :: row_counts(*), indices(*)
      real(c_double), intent(in) :: values(*); type(c_ptr), intent(out) :: plan
    end function
    integer(c_int) function sqmc_gpu_spmv_apply(plan, x, y, on_device) bind(C, name='sqmc_gpu_spmv_apply')
      import; type(c_ptr), value :: plan; real(c_double), intent(in) :: x(*); real(c_double), intent(out) :: y(*); integer(c_int), value :: on_device
    end function
    integer(c_int) function sqmc_gpu_spmv_free(plan) bind(C, name='sqmc_gpu_spmv_free')
      import; type(c_ptr), value :: plan
    end function
    integer(c_int) function sqmc_gpu_spmv_plan_submatrix(src, m, sel, dst, out_nnz_full) bind(C, name='sqmc_gpu_spmv_plan_submatrix')
      import; type(c_ptr), value :: src; integer(c_int64_t), value :: m; integer(c_int64_t), intent(in) :: sel(*)
      type(c_ptr), intent(out) :: dst; integer(c_int64_t), intent(out) :: out_nnz_full
    end function
    integer(c_int) function sqmc_shell_sort_magnitude(n, a, iorder) bind(C, name='sqmc_shell_sort_magnitude')
      import; integer(c_int64_t), value :: n; real(c_double), intent(inout) :: a(*); integer(c_int32_t), intent(inout) :: iorder(*)
    end function
    integer(c_int) function sqmc_gpu_spmv_sym_upper(n, row_counts, indices, values, x, y) bind(C, name='sqmc_gpu_spmv_sym_upper')
      import; integer(c_int64_t), value :: n; integer(c_int64_t), intent(in) :: row_counts(*), indices(*)
      real(c_double), intent(in) :: values(*), x(*); real(c_double), intent(out) :: y(*)
    end function
    integer(c_int) function sqmc_gpu_hamiltonian_batch(ctx, n, iu, id, ju, jd, h) bind(C, name='sqmc_gpu_hamiltonian_batch')
      import; type(c_ptr), value :: ctx; integer(c_int64_t), value :: n; integer(c_int64_t), intent(in) :: iu(*), id(*), ju(*), jd(*)
      real(c_double), intent(out) :: h(*)
    end function
    integer(c_int) function sqmc_gpu_hamiltonian_chem_batch(ctx, n, iu, id, ju, jd, h) bind(C, name='sqmc_gpu_hamiltonian_chem_batch')
      import; type(c_ptr), value :: ctx; integer(c_int64_t), value :: n; integer(c_int64_t), intent(in) :: iu(*), id(*), ju(*), jd(*)
      real(c_double), intent(out) :: h(*)
    end function
    integer(c_int) function sqmc_gpu_build_sparse_ham(ctx, n, up, dn, nnz, row_counts, indices, values) bind(C, name='sqmc_gpu_build_sparse_ham')
      import; type(c_ptr), value :: ctx; integer(c_int64_t), value :: n; integer(c_int64_t), intent(in) :: up(*), dn(*)
      integer(c_int64_t), intent(out) :: nnz; type(c_ptr), intent(out) :: row_counts, indices, values
    end function
    integer(c_int) function sqmc_gpu_propose_batch(ctx, n, tau, up, dn, seeds, ju, jd, weight_j, seeds_after) bind(C, name='sqmc_gpu_propose_batch')
      import; type(c_ptr), value :: ctx; integer(c_int64_t), value :: n; real(c_double), value :: tau
      integer(c_int64_t), intent(in) :: up(*), dn(*); integer(c_int32_t), intent(in) :: seeds(*)
      integer(c_int64_t), intent(out) :: ju(*), jd(*); real(c_double), intent(out) :: weight_j(*); integer(c_int32_t), intent(out) :: seeds_after(*)
    end function
    ! find_doubly_excited with the system's generator: find_important_connected_dets_chem / _heg, find_connected_dets_hubbard
    ! ('hubbard2': the hops in the reference's order, the source in slot 0, |H c| > eps) and find_connected_dets_hubbard_k ('hubbardk')
    integer(c_int) function sqmc_gpu_hci_connections(ctx, n_ref, ref_up, ref_dn, coeffs, eps, diag_mode, out_n, out_up, out_dn, out_num, out_den) &
        bind(C, name='sqmc_gpu_hci_connections')
      import; type(c_ptr), value :: ctx; integer(c_int64_t), value :: n_ref; integer(c_int64_t), intent(in) :: ref_up(*), ref_dn(*)
      real(c_double), intent(in) :: coeffs(*); real(c_double), value :: eps; integer(c_int), value :: diag_mode
      integer(c_int64_t), intent(out) :: out_n; type(c_ptr), intent(out) :: out_up, out_dn, out_num, out_den
    end function
    integer(c_int) function sqmc_gpu_hci_connections_slice(ctx, n_ref, ref_up, ref_dn, coeffs, eps, diag_mode, slice, n_slices, out_n, out_up, out_dn, &
        out_num, out_den) bind(C, name='sqmc_gpu_hci_connections_slice')
      import; type(c_ptr), value :: ctx; integer(c_int64_t), value :: n_ref; integer(c_int64_t), intent(in) :: ref_up(*), ref_dn(*)
      real(c_double), intent(in) :: coeffs(*); real(c_double), value :: eps; integer(c_int), value :: diag_mode
      integer(c_int32_t), value :: slice, n_slices
      integer(c_int64_t), intent(out) :: out_n; type(c_ptr), intent(out) :: out_up, out_dn, out_num, out_den
    end function
    subroutine sqmc_gpu_free(p) bind(C, name='sqmc_gpu_free')
      import; type(c_ptr), value :: p
    end subroutine
    integer(c_int) function sqmc_gpu_set_timing(ctx, on) bind(C, name='sqmc_gpu_set_timing')
      import; type(c_ptr), value :: ctx; integer(c_int), value :: on
    end function
    integer(c_int) function sqmc_gpu_get_timing(ctx, n, names, ms) bind(C, name='sqmc_gpu_get_timing')
      import; type(c_ptr), value :: ctx; integer(c_int32_t), intent(out) :: n; type(c_ptr), intent(out) :: names(*); real(c_float), intent(out) :: ms(*)
    end function
  end interface

contains

  !> Turns a non-zero status into the reference's way of failing: print the text and stop
  !> (the reference stops with these very texts: 'nwalk>MWALK' do_walk.f90:3690, 'my_nwalk=0' :2492, ...).
  subroutine sqmc_gpu_check(status, where)
    integer(c_int), intent(in) :: status
    character(len=*), intent(in) :: where
    character(kind=c_char), pointer :: msg(:)
    type(c_ptr) :: p
    integer :: i
    if (status == 0) return
    p = sqmc_gpu_last_error()
    write(6, '(a,a,a,i4)', advance='no') 'sqmc_gpu: ', where, ' failed with status', status
    if (c_associated(p)) then
      call c_f_pointer(p, msg, [512])
      write(6, '(a)', advance='no') ': '
      do i = 1, 512
        if (msg(i) == c_null_char) exit
        write(6, '(a)', advance='no') msg(i)
      enddo
    endif
    write(6, *)
    stop 'sqmc_gpu call failed'
  end subroutine

end module sqmc_gpu_mod
