! dazim_mc.f90 -- SurfDepthMC_amd: the Monte-Carlo second step of the two-step method.  It samples each map cell's Vs column with
! random-walk Metropolis chains on one MI355X and reports the posterior mean, spread and credible interval of every knot (DESIGN.md
! section 14), where SurfDepthFromMaps_amd returns one linearised model.
!
!   SurfDepthMC_amd para.in [nsample [nchain [width [sigma_c [seed [proposal [ntemp [tmax [aniso_thin [smooth_gcs [sigma_a
!                            [noise_a0 [noise_b0 [smooth_vs [damp_vs [types [radial [sigma_hv]]]]]]]]]]]]]]]]]]
!
! Inputs and weights are SurfDepthFromMaps_amd's: the unchanged para.in and MOD, period_phaseV_map.dat and, if present,
! period_map_coverage.dat (weight 1/sigma_c where DWS > 0, else 0).  Knots 1..nz-1 are sampled, the last one keeps MOD's value.
! Prior per cell and knot: uniform on [max(Minvel, MOD - width), min(Maxvel, MOD + width)]; width 0 (default) = [Minvel, Maxvel].
! nsample recorded steps (default 2000) after as many burn-in steps, nchain chains per cell (default 32), sigma_c 0.01 km/s, seed 1.
! proposal 0 (default): moves isotropic in box units; 1: moves shaped by the chains' own covariance, learnt per cell during burn-in
! and frozen afterwards (one more settings line and one more summary line: the cells with an adapted covariance).
! ntemp 1 (default): no tempering.  ntemp > 1 (a divisor of nchain): parallel tempering, every ntemp chains of a cell form a ladder
! of temperatures 1 .. tmax (default 16, geometric) whose neighbours swap states after every step; only the nchain / ntemp chains
! at temperature 1 are recorded (more settings lines, the swap acceptance over cells and rung pairs in the summary).
! aniso_thin 0 (default): Vs only, every file and byte as before.  aniso_thin > 0 (iso-mode F): the Gc/L, Gs/L posterior of every
! cell and knot from the chains themselves -- conditional on a Vs column the Gc/Gs posterior is the Gaussian of SurfDepthFromMaps_amd's
! column solve, and after every aniso_thin recorded steps its mean and covariance at the chains' current states join running sums
! (dazim_mc_set_aniso).  It reads period_Azm_tomo_map.inv (columns 8, 9) as SurfDepthFromMaps_amd does; weights 1/sigma_a (default
! sigma_c) where DWS > 0; smooth_gcs defaults to para.in's Gc/Gs smoothing weight, the damping is para.in's.  Two more files:
!   Gc_Gs_posterior_mc.dat       per inner cell and sampled knot: lon lat depth, Gc mean std, Gs mean std, the std_between of Gc and
!                                of Gs (the part of each std that comes from not knowing Vs), amplitude and its std, fast axis (degrees)
!                                and its std (write_azimuthal's arithmetic, the stds by the delta method), samples
!   Gc_Gs_model_mc.inv           the means on the posterior-mean Vs, as Gc_Gs_model.inv
! noise_a0 0 (default): the data std is sigma_c everywhere, every file and log line as before.  noise_a0 > 0: the data std of a cell
! becomes lambda * sigma_c with lambda unknown, lambda^2 ~ InverseGamma(noise_a0, noise_b0) a priori (noise_b0 defaults to 1);
! lambda is integrated out of the chains' target, so the Vs spreads carry the uncertainty of the noise level, and its posterior per
! cell comes back from the chains (dazim_mc_set_noise).  One more settings line, one more summary line, one more file:
!   noise_posterior_mc.dat       per inner cell: lon lat, mean and std of lambda, sigma_c * mean (the data std in km/s), periods
! smooth_vs 0 and damp_vs 0 (default): the uniform box is the whole prior, every file and log byte as before.  Otherwise the box
! truncates a Gaussian prior about MOD of precision smooth_vs^2 L^T L + damp_vs^2 I, SurfDepthFromMaps_amd's regulariser read as the
! prior its resolution output reads it as (dazim_mc_set_prior): Vs varies smoothly with depth about MOD, and the directions the
! periods do not resolve become proper.  One more settings line, one more summary line and, with noise_a0 0, one more file:
!   Vs_prior_check_mc.dat        per inner cell and sampled knot: lon lat depth, the chains' std, the linearised std_post of
!                                dazim_column_resolution at the posterior-mean model (its kernels, the run's weights, smooth_vs,
!                                damp_vs: SurfDepthFromMaps_amd's resolution block) and their ratio (0 where std_post is 0)
! With noise_a0 > 0 sigma_c is not the data std, the linearised std has nothing to stand on, and the file is not written.
! types 0 (default): a para.in that lists Rayleigh group or Love-wave periods is refused.  types 1: the maps of every wave type that
! para.in lists are sampled together (period_phaseV_map.dat as SurfPhaseMaps_amd writes it for typed data, one map per virtual
! period); the chains' forward model is dazim_dispersion_kernels_typed (dazim_mc_set_segments).  With noise_a0 > 0 every wave type
! gets a noise scale of its own, lambda_type^2 ~ InverseGamma(noise_a0, noise_b0) each (dazim_mc_set_noise_groups):
! noise_posterior_mc.dat then holds one block per type, its lines ending in the type's wavetp veltp, period_phaseV_mc.dat ends in
! those two columns as every typed map file does, and the log gets one line per type: its periods, the mean |c residual| of the
! best model and the median lambda.  aniso_thin > 0 is refused with typed data: the Gc/Gs kernel Lsen_Gsc is Rayleigh-phase.
! Rayleigh-phase input writes the same bytes with types 0 and 1.
! radial 0 (default): one Vs profile per cell, every file and log byte as before.  radial 1 (needs types 1, Rayleigh and Love periods
! in para.in, aniso_thin 0 and nz - 1 <= 31): radial anisotropy (DESIGN.md sections 13.1 and 14.2).  The chains sample Vsv and Vsh
! together (dazim_mc_set_radial): the Rayleigh maps see Vsv, the Love maps Vsh, both profiles start from MOD and share its box, the
! deepest knot is MOD's for both, and the prior gains (Vsh - Vsv)^2 / sigma_hv^2 per knot (sigma_hv default 0.2 km/s; 0: no
! coupling).  smooth_vs and damp_vs act on each profile about MOD.  MOD_mc, DSurfTomo_mc.inv and Vs_posterior_mc.dat then hold Vsv,
! period_phaseV_mc.dat the Rayleigh periods of the mean Vsv and the Love periods of the mean Vsh, cell_mc.dat's misfits are those of
! the two best and the two mean profiles, and there are more files:
!   MOD_Vsh_mc, Vsh_posterior_mc.dat   the posterior mean of Vsh and its statistics, as MOD_mc and Vs_posterior_mc.dat
!   xi_posterior_mc.dat          per inner cell and sampled knot: lon lat depth, xi = (Vsh / Vsv)^2 mean std p2.5 p50 p97.5 R-hat
!                                P(xi > 1), the Vsv-Vsh correlation of the chains, the Voigt average sqrt((2 Vsv^2 + Vsh^2) / 3) mean std
!   Vsv_Vsh_model_mc.inv         the posterior means on the whole grid, as Vsv_Vsh_model_2step.inv; its xi is the posterior mean of xi
!   Vsv_Vsh_prior_check_mc.dat   (smooth_vs or damp_vs > 0, noise_a0 0) per inner cell and sampled knot: lon lat depth, then for Vsv
!                                and for Vsh the chains' std, dazim_column_resolution_radial's std at the posterior-mean models and
!                                their ratio (0 where the linearised std is 0)
! The log gains the settings line, R-hat of xi and the share of sampled (cell, knot)s whose P(xi > 1) lies outside [0.025, 0.975].
!
! Outputs (names of their own, so that the three programs can share a directory):
!   MOD_mc, DSurfTomo_mc.inv     the posterior mean, as MOD_2step and DSurfTomo_2step.inv
!   Vs_posterior_mc.dat          per inner cell and sampled knot: lon lat depth mean std p2.5 p50 p97.5 best R-hat
!   period_phaseV_mc.dat         c of the posterior-mean model, as period_phaseV_map.dat
!   cell_mc.dat                  per inner cell: lon lat acceptance, RMS c misfit of the best and of the mean model
!   <para>_mc.log + stdout       settings, cells, proposals without a root, acceptance quartiles, R-hat, misfit
program SurfDepthMC_amd
  use iso_c_binding
  use dazim_mod
  use dazim_io
  implicit none
  integer, parameter :: nbin = 200, nadapt = 50
  real, parameter :: step0 = 0.05
  character(len=100) :: inputfile, logfile
  type(para_t) :: p
  logical :: ex
  integer :: nx, ny, nz, kmax, nsample, nchain, proposal, ntemp, ncold, aniso_thin
  real :: smooth_gcs, sigma_a, t_aniso, gc, gs, g2, vcc, vss, vcs, amp, samp, sang
  real, allocatable :: amap(:, :, :, :), wa(:, :, :), gmean(:, :, :, :), gstd(:, :, :, :), gstdb(:, :, :, :), gcov(:, :, :)
  integer(c_int64_t), allocatable :: nsamp(:, :)
  integer :: npass, nskip
  real :: noise_a0, noise_b0
  real :: smooth_vs, damp_vs
  logical :: prior_on
  real*8, allocatable, target :: svs(:, :, :), svp(:, :, :), srho(:, :, :), skern(:, :, :)
  real*8, allocatable :: pvk(:, :)
  real, allocatable :: res(:, :, :, :), rtrace(:, :), ratio(:, :, :)
  integer(c_int) :: nempty_res, nbad
  real, allocatable :: lam_mean(:, :), lam_std(:, :)
  integer(c_int), allocatable :: ndata(:, :)
  integer :: types, ngrp, g, wavetp, veltp
  logical :: typed
  integer(c_int), allocatable :: grp(:)
  real(c_float) :: ga0(4), gb0(4)
  real, allocatable :: glam_mean(:, :, :), glam_std(:, :, :)
  integer(c_int), allocatable :: gndata(:, :, :)
  integer, parameter :: nswap = 1
  integer :: radial
  real :: sigma_hv
  real :: tmax
  real(c_double), allocatable, target :: beta(:)
  integer(c_int64_t), allocatable, target :: swap_try(:, :), swap_acc(:, :)
  integer(c_long_long) :: seed
  real :: goxd, gozd, dvxd, dvzd, minthk, Minvel, Maxvel, width, sigma_c
  real*8, allocatable :: tRc(:)
  real, allocatable :: depz(:), vsf(:, :, :), vmc(:, :, :), vbest(:, :, :)
  real*8, allocatable :: pvm(:, :), pvb(:, :)
  real, allocatable :: cmap(:, :, :), wcov(:, :, :), vmin(:, :, :), vmax(:, :, :)
  real, allocatable :: mean(:, :, :), std(:, :, :), qq(:, :, :, :), best(:, :, :), rhat(:, :, :), acc(:, :), chi2b(:, :)
  real, allocatable :: sorted(:), rms_b(:, :), rms_m(:, :)
  logical, allocatable :: sampled(:, :)
  real :: rms_all, t_run, t_disp, t_step
  real*8 :: s0, cnt
  integer :: i, j, k, t, nlay, ncell, q, ns, nr, ncov
  integer(c_int) :: nfail, nempty
  integer(c_int64_t) :: nnoroot
  type(c_ptr) :: mc

  write (*, *)
  write (*, *) '                       SurfDepthMC'
  write (*, *)
  if (command_argument_count() < 1) error stop &
    'usage: SurfDepthMC_amd para.in [nsample [nchain [width [sigma_c [seed [proposal [ntemp [tmax [aniso_thin [smooth_gcs [sigma_a '// &
    '[noise_a0 [noise_b0 [smooth_vs [damp_vs [types [radial [sigma_hv]]]]]]]]]]]]]]]]]]'
  call get_command_argument(1, inputfile)
  inquire (file=inputfile, exist=ex)
  if (.not. ex) error stop 'unable to open the inputfile'
  call read_para(inputfile, p)
  nx = p%nx; ny = p%ny; nz = p%nz; goxd = p%goxd; gozd = p%gozd; dvxd = p%dvxd; dvzd = p%dvzd; minthk = p%minthk
  Minvel = p%Minvel; Maxvel = p%Maxvel; kmax = p%kmaxRc; tRc = p%tRc
  if (nz <= 1) error stop 'error nz value.'
  if (kmax <= 0) error stop 'Can only deal with Rayleigh wave phase velocity data!'
  types = 0
  call optional_arg(17, types)
  if (types /= 0 .and. types /= 1) error stop 'types must be 0 or 1'
  if (p%typed .and. types == 0) then
    write (*, '(a)') ' ERROR: SurfDepthMC_amd: para.in lists Rayleigh group or Love-wave periods; the Monte-Carlo forward model is the'
    write (*, '(a)') ' Rayleigh phase-velocity kernel.  Use SurfDepthFromMaps_amd for maps of other wave types.'
    write (*, '(a)') ' Or pass types = 1, the sixteenth argument after para.in, to sample the maps of every wave type together.'
    error stop 'SurfDepthMC_amd takes Rayleigh phase velocities only'
  end if
  typed = p%typed
  nsample = 2000; nchain = 32; width = 0; sigma_c = 0.01; seed = 1; proposal = 0; ntemp = 1; tmax = 16
  call optional_arg(2, nsample)
  call optional_arg(3, nchain)
  call optional_arg(4, width)
  call optional_arg(5, sigma_c)
  call optional_arg(6, seed)
  call optional_arg(7, proposal)
  call optional_arg(8, ntemp)
  call optional_arg(9, tmax)
  aniso_thin = 0; smooth_gcs = p%weightGcs
  call optional_arg(10, aniso_thin)
  call optional_arg(11, smooth_gcs)
  sigma_a = sigma_c
  call optional_arg(12, sigma_a)
  noise_a0 = 0; noise_b0 = 1
  call optional_arg(13, noise_a0)
  call optional_arg(14, noise_b0)
  smooth_vs = 0; damp_vs = 0
  call optional_arg(15, smooth_vs)
  call optional_arg(16, damp_vs)
  if (nsample < 1) error stop 'nsample must be at least 1'
  if (nchain < 1 .or. nchain > 64) error stop 'nchain must be 1..64'
  if (width < 0) error stop 'width must not be negative'
  if (sigma_c <= 0) error stop 'sigma_c must be positive'
  if (proposal /= 0 .and. proposal /= 1) error stop 'proposal must be 0 or 1'
  if (ntemp < 1 .or. ntemp > nchain) error stop 'ntemp must be 1..nchain and divide nchain'
  if (mod(nchain, ntemp) /= 0) error stop 'ntemp must be 1..nchain and divide nchain'
  if (ntemp > 1 .and. .not. (tmax > 1 .and. tmax <= huge(tmax))) error stop 'tmax must be a finite temperature above 1'
  if (aniso_thin < 0) error stop 'aniso_thin must not be negative'
  if (aniso_thin > 0 .and. typed) then
    write (*, '(a)') ' ERROR: aniso_thin > 0 with types = 1: para.in lists Rayleigh group or Love-wave periods, and the Gc/Gs kernel'
    write (*, '(a)') ' (Lsen_Gsc) exists for Rayleigh phase velocities only.'
    error stop 'aniso_thin > 0 takes Rayleigh phase velocities only'
  end if
  if (aniso_thin > 0 .and. p%iso_mod) then
    write (*, '(a)') ' ERROR: aniso_thin > 0 needs the 2-psi maps of iso-mode F; para.in has iso-mode T'
    error stop 'aniso_thin > 0 with iso-mode T'
  end if
  if (aniso_thin > 0 .and. sigma_a <= 0) error stop 'sigma_a must be positive'
  if (aniso_thin > 0 .and. (smooth_gcs < 0 .or. (smooth_gcs == 0 .and. p%damp == 0))) error stop &
    'smooth_gcs must not be negative, nor 0 together with para.in''s damping'
  if (.not. (noise_a0 >= 0 .and. noise_a0 <= huge(noise_a0))) error stop 'noise_a0 must not be negative'
  if (noise_a0 > 0 .and. .not. (noise_b0 > 0 .and. noise_b0 <= huge(noise_b0))) error stop 'noise_b0 must be positive'
  if (.not. (smooth_vs >= 0 .and. smooth_vs <= huge(smooth_vs))) error stop 'smooth_vs must be finite and not negative'
  if (.not. (damp_vs >= 0 .and. damp_vs <= huge(damp_vs))) error stop 'damp_vs must be finite and not negative'
  prior_on = smooth_vs > 0 .or. damp_vs > 0
  radial = 0; sigma_hv = 0.2
  call optional_arg(18, radial)
  call optional_arg(19, sigma_hv)
  if (radial /= 0 .and. radial /= 1) error stop 'radial must be 0 or 1'
  if (radial == 1) then
    if (types /= 1) then
      write (*, '(a)') ' ERROR: radial = 1 needs types = 1: Vsv comes from the Rayleigh maps and Vsh from the Love maps.'
      error stop 'radial = 1 needs types = 1'
    end if
    if (sum(p%type_kmax(3:4)) == 0) then
      write (*, '(a)') ' ERROR: radial = 1: para.in lists no Love periods (kmaxLc, kmaxLg); Vsh is what the Love maps constrain.'
      error stop 'radial = 1 needs Love periods'
    end if
    if (sum(p%type_kmax(1:2)) == 0) then
      write (*, '(a)') ' ERROR: radial = 1: para.in lists no Rayleigh periods (kmaxRc, kmaxRg); Vsv is what the Rayleigh maps constrain.'
      error stop 'radial = 1 needs Rayleigh periods'
    end if
    if (aniso_thin > 0) then
      write (*, '(a)') ' ERROR: radial = 1 with aniso_thin > 0: Gc/Gs together with radial anisotropy is not supported.'
      error stop 'radial = 1 needs aniso_thin = 0'
    end if
    if (nz - 1 > 31) then
      write (*, '(a)') ' ERROR: radial = 1 samples 2 (nz - 1) knots per cell, 62 at most: nz <= 32.'
      error stop 'radial = 1 needs nz - 1 <= 31'
    end if
    if (.not. (sigma_hv >= 0 .and. sigma_hv <= huge(sigma_hv))) error stop 'sigma_hv must be finite and not negative'
  end if
  ncold = nchain/ntemp
  nlay = nz - 1
  ncell = (nx - 2)*(ny - 2)
  if (nlay > 63) error stop 'SurfDepthMC_amd samples at most 63 knots (nz <= 64)'
  if (kmax > 60) error stop 'SurfDepthMC_amd takes at most 60 periods'
  if (typed) call dazim_set_segments(p%nseg, p%seg_wavetp, p%seg_veltp, p%seg_kmax)
  if (.not. (Minvel < Maxvel)) error stop 'para.in''s Vs range is empty'
  write (logfile, '(a,a)') trim(inputfile), '_mc.log'
  open (66, file=logfile)
  write (66, *)
  write (66, *) '                  SurfDepthMC'
  write (66, *)
  do q = 6, 66, 60
    write (q, '(a,3i5,a,i3,a)') ' grid nx ny nz:', nx, ny, nz, ';', kmax, ' periods'
    write (q, '(a,50f6.1)') ' periods (s):', (tRc(i), i=1, kmax)
    write (q, '(a,i7,a,i7,a,i3,a,i20)') ' recorded steps', nsample, '  burn-in steps', nsample, '  chains per cell', nchain, &
      '  seed', seed
    write (q, '(a,f8.4,a,f8.3,a,i4,a,i4)') ' sigma_c (km/s)', sigma_c, '  initial step scale', step0, '  adaptation every', &
      nadapt, ' burn-in steps;  histogram bins', nbin
    if (width > 0) then
      write (q, '(a,f8.4,a,2f8.3)') ' prior: uniform on MOD +-', width, ' km/s inside para.in''s Vs range', Minvel, Maxvel
    else
      write (q, '(a,2f8.3)') ' prior: uniform on para.in''s Vs range', Minvel, Maxvel
    end if
    if (proposal == 1) write (q, '(a)') ' proposal 1: shaped by the chains'' covariance, learnt per cell during burn-in'
    if (ntemp > 1) write (q, '(a,i3,a,f9.3,a,i3,a,i3,a)') ' parallel tempering:', ntemp, ' rungs up to T =', tmax, &
      ', a swap round every', nswap, ' step(s);', ncold, ' chains per cell at T = 1 are recorded'
    if (aniso_thin > 0) write (q, '(a,i6,a,f8.3,a,f8.3,a,f8.4)') ' Gc/Gs posteriors: one sample of every recorded chain per', &
      aniso_thin, ' recorded steps;  smoothing', smooth_gcs, '  damping', p%damp, '  sigma_a (km/s)', sigma_a
    if (typed) then
      do g = 1, p%nseg
        write (q, '(a,a,a,i3,a,i3)') ' wave type ', trim(type_name(p%seg_wavetp(g), p%seg_veltp(g))), ':', p%seg_kmax(g), &
          ' periods from virtual period', sum(p%seg_kmax(1:g - 1)) + 1
      end do
    end if
    if (noise_a0 > 0 .and. typed) then
      write (q, '(a,f9.4,a,f9.4,a)') ' hierarchical noise: data std lambda_type * sigma_c per cell and wave type, each lambda^2 ~ '// &
        'InverseGamma(', noise_a0, ',', noise_b0, '), integrated out of the chains'' target'
    else if (noise_a0 > 0) then
      write (q, '(a,f9.4,a,f9.4,a)') ' hierarchical noise: data std lambda * sigma_c per cell, lambda^2 ~ InverseGamma(', &
        noise_a0, ',', noise_b0, '), integrated out of the chains'' target'
    end if
    if (prior_on) write (q, '(a,f8.3,a,f8.3,a)') ' Gaussian prior about MOD inside the box: smoothing', smooth_vs, '  damping', &
      damp_vs, ' (precision smooth^2 L^T L + damp^2 I)'
    if (radial == 1) write (q, '(a,i3,a,i3,a,f8.4)') ' radial anisotropy: Vsv from the', sum(p%type_kmax(1:2)), &
      ' Rayleigh periods, Vsh from the', sum(p%type_kmax(3:4)), ' Love periods, both from MOD; sigma_hv (km/s)', sigma_hv
  end do

  call read_mod('MOD', p, depz, vsf)

  ! ---- the maps and the weights (SurfDepthFromMaps_amd's) ------------------------------------------------------------------------
  allocate (cmap(nx - 2, ny - 2, kmax), wcov(nx - 2, ny - 2, kmax))
  call read_map('period_phaseV_map.dat', p, 4, 4, cmap, .true.)
  call coverage_weights(p, sigma_c, wcov)
  if (aniso_thin > 0) then
    allocate (amap(nx - 2, ny - 2, kmax, 2), wa(nx - 2, ny - 2, kmax))
    call read_map('period_Azm_tomo_map.inv', p, 9, 8, amap(:, :, :, 1), .true.)
    call read_map('period_Azm_tomo_map.inv', p, 9, 9, amap(:, :, :, 2), .false.)
    wa = merge(1.0/sigma_a, 0.0, wcov /= 0.0)
  end if

  ! ---- the prior box per cell and knot -------------------------------------------------------------------------------------------
  allocate (vmin(nx - 2, ny - 2, nlay), vmax(nx - 2, ny - 2, nlay))
  if (width > 0) then
    vmin = max(Minvel, vsf(2:nx - 1, 2:ny - 1, 1:nlay) - width)
    vmax = min(Maxvel, vsf(2:nx - 1, 2:ny - 1, 1:nlay) + width)
  else
    vmin = Minvel
    vmax = Maxvel
  end if
  if (any(.not. (vmin < vmax))) then
    write (*, '(a)') ' ERROR: MOD lies outside para.in''s Vs range by more than width: an empty prior box'
    error stop 'empty prior box'
  end if

  if (radial == 1) then
    call radial_run()
    write (*, *) '  Program finishes successfully'
    write (66, *) '  Program finishes successfully'
    close (66)
    call dazim_finalize()
    stop
  end if

  ! ---- the chains ----------------------------------------------------------------------------------------------------------------
  call dazim_init(0)
  call dazim_check(dazim_mc_create(dazim_handle, nx, ny, nz, kmax, nchain, nbin, seed, vsf, vmin, vmax, cmap, wcov, step0, nadapt, &
                                   mc, nempty), 'Monte-Carlo chains')
  do q = 6, 66, 60
    write (q, '(a,i8,a,i8)') ' cells sampled', ncell - nempty, '  cells without data (start model kept)', nempty
  end do
  if (proposal /= 0) call dazim_check(dazim_mc_set_proposal(dazim_handle, mc, proposal), 'Monte-Carlo proposal')
  if (ntemp > 1) then
    allocate (beta(ntemp), swap_try(ntemp - 1, ncell - nempty), swap_acc(ntemp - 1, ncell - nempty))
    call dazim_check(dazim_mc_set_tempering(dazim_handle, mc, ntemp, tmax, nswap), 'Monte-Carlo tempering')
    call dazim_check(dazim_mc_temper_state(dazim_handle, mc, c_null_ptr, c_null_ptr, c_null_ptr, c_loc(beta), c_null_ptr, &
                                           c_null_ptr, c_null_ptr), 'tempering ladder')
    do q = 6, 66, 60
      write (q, '(a,64f8.3)') ' ladder, temperatures 1 / beta:', (1.0d0/beta(i), i=1, ntemp)
    end do
  end if
  if (aniso_thin > 0) call dazim_check(dazim_mc_set_aniso(dazim_handle, mc, aniso_thin, amap, wa, smooth_gcs, p%damp), &
                                       'Gc/Gs posteriors')
  ngrp = 0
  if (typed) then
    call dazim_check(dazim_mc_set_segments(dazim_handle, mc, p%nseg, p%seg_wavetp, p%seg_veltp, p%seg_kmax), 'wave types')
    if (noise_a0 > 0) then                    ! one noise scale per wave type: the group of a period is its segment
      ngrp = p%nseg
      allocate (grp(kmax))
      do g = 1, ngrp
        grp(sum(p%seg_kmax(1:g - 1)) + 1:sum(p%seg_kmax(1:g))) = g - 1
      end do
      ga0 = noise_a0; gb0 = noise_b0
      call dazim_check(dazim_mc_set_noise_groups(dazim_handle, mc, ngrp, grp, ga0, gb0), 'hierarchical noise per wave type')
    end if
  else if (noise_a0 > 0) then
    call dazim_check(dazim_mc_set_noise(dazim_handle, mc, noise_a0, noise_b0), 'hierarchical noise')
  end if
  if (prior_on) call dazim_check(dazim_mc_set_prior(dazim_handle, mc, smooth_vs, damp_vs, c_null_ptr), 'Gaussian prior')
  call dazim_check(dazim_mc_run(dazim_handle, mc, depz, minthk, tRc, nsample, nsample, nnoroot), 'Monte-Carlo run')
  t_run = real(dazim_last_kernel_seconds(dazim_handle, 'mc'//c_null_char))
  t_disp = real(dazim_last_kernel_seconds(dazim_handle, 'mc.disp'//c_null_char))
  t_step = real(dazim_last_kernel_seconds(dazim_handle, 'mc.step'//c_null_char))
  ncov = nint(dazim_last_kernel_seconds(dazim_handle, 'mc.cov_cells'//c_null_char))
  allocate (mean(nx - 2, ny - 2, nlay), std(nx - 2, ny - 2, nlay), qq(nx - 2, ny - 2, nlay, 3), best(nx - 2, ny - 2, nlay))
  allocate (rhat(nx - 2, ny - 2, nlay), acc(nx - 2, ny - 2), chi2b(nx - 2, ny - 2))
  call dazim_check(dazim_mc_result(dazim_handle, mc, mean, std, qq, best, rhat, acc, chi2b), 'posterior statistics')
  if (ntemp > 1) call dazim_check(dazim_mc_temper_state(dazim_handle, mc, c_null_ptr, c_null_ptr, c_null_ptr, c_null_ptr, &
                                                        c_null_ptr, c_loc(swap_try), c_loc(swap_acc)), 'swap counts')
  if (aniso_thin > 0) then
    t_aniso = real(dazim_last_kernel_seconds(dazim_handle, 'mc.aniso'//c_null_char))
    npass = nint(dazim_last_kernel_seconds(dazim_handle, 'mc.aniso_passes'//c_null_char))
    nskip = nint(dazim_last_kernel_seconds(dazim_handle, 'mc.aniso_skipped'//c_null_char))
    allocate (gmean(nx - 2, ny - 2, nlay, 2), gstd(nx - 2, ny - 2, nlay, 2), gstdb(nx - 2, ny - 2, nlay, 2))
    allocate (gcov(nx - 2, ny - 2, nlay), nsamp(nx - 2, ny - 2))
    if (npass > 0) then
      call dazim_check(dazim_mc_aniso_result(dazim_handle, mc, gmean, gstd, gstdb, gcov, nsamp), 'Gc/Gs posterior statistics')
    else   ! fewer recorded steps than aniso_thin: no sample
      gmean = 0; gstd = 0; gstdb = 0; gcov = 0; nsamp = 0
    end if
  end if
  if (ngrp > 0) then
    allocate (glam_mean(nx - 2, ny - 2, ngrp), glam_std(nx - 2, ny - 2, ngrp), gndata(nx - 2, ny - 2, ngrp))
    call dazim_check(dazim_mc_noise_groups_result(dazim_handle, mc, glam_mean, glam_std, gndata), 'noise-scale posteriors')
  else if (noise_a0 > 0) then
    allocate (lam_mean(nx - 2, ny - 2), lam_std(nx - 2, ny - 2), ndata(nx - 2, ny - 2))
    call dazim_check(dazim_mc_noise_result(dazim_handle, mc, lam_mean, lam_std, ndata), 'noise-scale posterior')
  end if
  call dazim_check(dazim_mc_free(dazim_handle, mc), 'Monte-Carlo chains')

  ! ---- the curves of the mean and of the best model ------------------------------------------------------------------------------
  allocate (vmc(nx, ny, nz), vbest(nx, ny, nz), pvm(nx*ny, kmax), pvb(nx*ny, kmax))
  vmc = vsf; vbest = vsf
  vmc(2:nx - 1, 2:ny - 1, 1:nlay) = mean
  vbest(2:nx - 1, 2:ny - 1, 1:nlay) = best
  call dazim_check(dazim_dispersion_any(dazim_handle, nx, ny, nz, vmc, depz, minthk, kmax, tRc, pvm, c_null_ptr, c_null_ptr, &
                                        c_null_ptr, nfail), 'dispersion curves of the mean model')
  call dazim_check(dazim_dispersion_any(dazim_handle, nx, ny, nz, vbest, depz, minthk, kmax, tRc, pvb, c_null_ptr, c_null_ptr, &
                                        c_null_ptr, nfail), 'dispersion curves of the best model')
  allocate (rms_b(nx - 2, ny - 2), rms_m(nx - 2, ny - 2), sampled(nx - 2, ny - 2))
  sampled = any(wcov /= 0.0, dim=3)
  ! ---- the chains' std against the linearised std_post at the posterior-mean model (SurfDepthFromMaps_amd's resolution block) ------
  if (prior_on .and. .not. noise_a0 > 0) then
    allocate (svs(nx*ny, kmax, nz), svp(nx*ny, kmax, nz), srho(nx*ny, kmax, nz), skern(nx*ny, kmax, nz), pvk(nx*ny, kmax))
    allocate (res(nx - 2, ny - 2, nlay, 5), rtrace(nx - 2, ny - 2), ratio(nx - 2, ny - 2, nlay))
    call dazim_check(dazim_dispersion_any(dazim_handle, nx, ny, nz, vmc, depz, minthk, kmax, tRc, pvk, c_loc(svs), c_loc(svp), &
                                          c_loc(srho), nfail), 'depth kernels of the mean model')
    call dazim_check(dazim_vs_kernels(dazim_handle, nx, ny, nz, kmax, vmc, svs, svp, srho, skern), 'dc/dVs table of the mean model')
    call dazim_check(dazim_column_resolution(dazim_handle, nx, ny, nlay, kmax, 0, c_loc(skern), wcov, smooth_vs, damp_vs, depz, &
                                             res(:, :, :, 1), res(:, :, :, 2), res(:, :, :, 3), res(:, :, :, 4), res(:, :, :, 5), &
                                             c_null_ptr, rtrace, nempty_res, nbad), 'column resolution at the mean model')
    ratio = 0
    where (res(:, :, :, 1) > 0) ratio = std/res(:, :, :, 1)
  end if
  s0 = 0; cnt = 0
  do j = 1, ny - 2
    do i = 1, nx - 2
      rms_b(i, j) = cell_rms(pvb, i, j)
      rms_m(i, j) = cell_rms(pvm, i, j)
      do t = 1, kmax
        if (wcov(i, j, t) /= 0.0) then
          s0 = s0 + (real(cmap(i, j, t), 8) - pvm(j*nx + i + 1, t))**2
          cnt = cnt + 1
        end if
      end do
    end do
  end do
  rms_all = 0
  if (cnt > 0) rms_all = real(sqrt(s0/cnt))

  ! ---- summary -------------------------------------------------------------------------------------------------------------------
  ns = count(sampled)
  do q = 6, 66, 60
    write (q, '(a,i12,a,i12)') ' proposals without a root:', nnoroot, ' of', int(2*nsample, 8)*ns*nchain
    write (q, '(a,f9.2,a,f9.2,a,f9.3,a)') ' run', t_run, ' s (dispersion calls', t_disp, ' s, step kernels', t_step, ' s)'
    if (proposal == 1) write (q, '(a,i8,a,i8)') ' cells with an adapted covariance:', ncov, ' of', ns
  end do
  if (aniso_thin > 0) then
    nr = count(spread(spread(nsamp > 0, 3, nlay), 4, 2) .and. gstd > 0)
    allocate (sorted(max(nr, 1)))
    sorted = 0
    if (nr > 0) sorted(1:nr) = pack(gstdb/max(gstd, tiny(1.0)), spread(spread(nsamp > 0, 3, nlay), 4, 2) .and. gstd > 0)
    call sort(sorted)
    do q = 6, 66, 60
      write (q, '(a,i7,a,i9,a,f9.2,a)') ' Gc/Gs passes', npass, '  skipped states', nskip, '  in', t_aniso, ' s'
      write (q, '(a,f8.4)') ' Gc/Gs: median over (cell, knot) of std_between / std, the share of the Vs uncertainty:', &
        sorted(max(1, (nr + 1)/2))
    end do
    deallocate (sorted)
  end if
  if (ntemp > 1 .and. ns > 0) then
    nr = count(swap_try > 0)
    allocate (sorted(max(nr, 1)))
    sorted = 0
    if (nr > 0) sorted(1:nr) = pack(real(swap_acc)/real(max(swap_try, 1_c_int64_t)), swap_try > 0)
    call sort(sorted)
    do q = 6, 66, 60
      write (q, '(a,4f8.3)') ' swap acceptance over (cell, rung pair), minimum and quartiles 25/50/75 %:', sorted(1), &
        sorted(max(1, nint(0.25*nr))), sorted(max(1, nint(0.5*nr))), sorted(max(1, nint(0.75*nr)))
      write (q, '(a,i3,a,i3,a)') ' the statistics below are of the', ncold, ' chains per cell at T = 1 (of', nchain, ')'
    end do
    deallocate (sorted)
  end if
  if (ns > 0) then
    allocate (sorted(ns))
    sorted = pack(acc, sampled)
    call sort(sorted)
    do q = 6, 66, 60
      write (q, '(a,3f8.3)') ' acceptance over cells, quartiles 25/50/75 %:', sorted(max(1, nint(0.25*ns))), &
        sorted(max(1, nint(0.5*ns))), sorted(max(1, nint(0.75*ns)))
    end do
    deallocate (sorted)
    nr = count(spread(sampled, 3, nlay) .and. rhat == rhat)
    allocate (sorted(max(nr, 1)))
    sorted = 0
    if (nr > 0) sorted(1:nr) = pack(rhat, spread(sampled, 3, nlay) .and. rhat == rhat)
    call sort(sorted(1:max(nr, 1)))
    do q = 6, 66, 60
      write (q, '(a,2f9.4)') ' R-hat over (cell, knot), median and maximum:', sorted(max(1, (nr + 1)/2)), sorted(max(nr, 1))
    end do
  end if
  if (typed) then   ! per wave type: its periods, the mean |c residual| of the best model and, with the noise scales, the median lambda
    do g = 1, p%nseg
      s0 = 0; cnt = 0
      do t = sum(p%seg_kmax(1:g - 1)) + 1, sum(p%seg_kmax(1:g))
        do j = 1, ny - 2
          do i = 1, nx - 2
            if (wcov(i, j, t) /= 0.0) then
              s0 = s0 + abs(real(cmap(i, j, t), 8) - pvb(j*nx + i + 1, t))
              cnt = cnt + 1
            end if
          end do
        end do
      end do
      if (cnt > 0) s0 = s0/cnt
      if (allocated(sorted)) deallocate (sorted)
      nr = 0
      if (ngrp > 0) nr = count(gndata(:, :, g) > 0 .and. glam_mean(:, :, g) == glam_mean(:, :, g))
      allocate (sorted(max(nr, 1)))
      sorted = 0
      if (nr > 0) sorted(1:nr) = pack(glam_mean(:, :, g), gndata(:, :, g) > 0 .and. glam_mean(:, :, g) == glam_mean(:, :, g))
      call sort(sorted)
      do q = 6, 66, 60
        if (ngrp > 0) then
          write (q, '(a,a,a,i3,a,f10.5,a,f9.3)') ' ', trim(type_name(p%seg_wavetp(g), p%seg_veltp(g))), ':', p%seg_kmax(g), &
            ' periods, best model mean |c residual| (km/s)', s0, ', median of the mean of lambda over cells', sorted(max(1, (nr + 1)/2))
        else
          write (q, '(a,a,a,i3,a,f10.5)') ' ', trim(type_name(p%seg_wavetp(g), p%seg_veltp(g))), ':', p%seg_kmax(g), &
            ' periods, best model mean |c residual| (km/s)', s0
        end if
      end do
      deallocate (sorted)
    end do
  end if
  if (noise_a0 > 0 .and. ngrp == 0) then
    nr = count(sampled .and. lam_mean == lam_mean)
    if (allocated(sorted)) deallocate (sorted)
    allocate (sorted(max(nr, 1)))
    sorted = 0
    if (nr > 0) sorted(1:nr) = pack(lam_mean, sampled .and. lam_mean == lam_mean)
    call sort(sorted)
    do q = 6, 66, 60
      write (q, '(a,5f9.3)') ' noise scale over cells (mean of lambda), minimum, quartiles 25/50/75 % and maximum:', sorted(1), &
        sorted(max(1, nint(0.25*nr))), sorted(max(1, nint(0.5*nr))), sorted(max(1, nint(0.75*nr))), sorted(max(nr, 1))
    end do
    deallocate (sorted)
  end if
  if (prior_on .and. noise_a0 > 0) then
    do q = 6, 66, 60
      write (q, '(a)') ' Gaussian prior: Vs_prior_check_mc.dat is not written, with the noise scale unknown sigma_c is not the data std'
    end do
  else if (prior_on) then
    nr = count(spread(sampled, 3, nlay) .and. ratio > 0)
    if (allocated(sorted)) deallocate (sorted)
    allocate (sorted(max(nr, 1)))
    sorted = 0
    if (nr > 0) sorted(1:nr) = pack(ratio, spread(sampled, 3, nlay) .and. ratio > 0)
    call sort(sorted)
    do q = 6, 66, 60
      write (q, '(a,3f9.4)') ' Gaussian prior: chains'' std / linearised std_post over (cell, knot), quartiles 25/50/75 %:', &
        sorted(max(1, nint(0.25*nr))), sorted(max(1, (nr + 1)/2)), sorted(max(1, nint(0.75*nr)))
    end do
    deallocate (sorted)
  end if
  do q = 6, 66, 60
    write (q, '(a,f12.5)') ' posterior-mean model: rms_c', rms_all
  end do

  ! ---- output files --------------------------------------------------------------------------------------------------------------
  call write_mod('MOD_mc', depz, vmc)
  call write_vs_model('DSurfTomo_mc.inv', p, depz, vmc)
  open (64, file='Vs_posterior_mc.dat')
  do k = 1, nlay
    do j = 1, ny - 2
      do i = 1, nx - 2
        write (64, '(3f10.4,7f10.4)') gozd + (j - 1)*dvzd, goxd - (i - 1)*dvxd, depz(k), mean(i, j, k), std(i, j, k), &
          qq(i, j, k, 1), qq(i, j, k, 2), qq(i, j, k, 3), best(i, j, k), rhat(i, j, k)
      end do
    end do
  end do
  close (64)
  call write_phase_map('period_phaseV_mc.dat', p, inner_cells(nx, ny, kmax, pvm))
  if (aniso_thin > 0) then
    call write_azimuthal('Gc_Gs_model_mc.inv', p, depz, vmc, gmean(:, :, :, 1), gmean(:, :, :, 2))
    open (64, file='Gc_Gs_posterior_mc.dat')
    do k = 1, nlay
      do j = 1, ny - 2
        do i = 1, nx - 2
          ! amplitude and fast axis as write_azimuthal forms them; their stds by the delta method from the Gc/Gs covariance
          gc = gmean(i, j, k, 1); gs = gmean(i, j, k, 2)
          vcc = gstd(i, j, k, 1)**2; vss = gstd(i, j, k, 2)**2; vcs = gcov(i, j, k)
          g2 = gc**2 + gs**2
          amp = 0.5*sqrt(g2)
          samp = 0; sang = 0
          if (g2 > 0) then
            samp = 0.5*sqrt(max((gc**2*vcc + 2*gc*gs*vcs + gs**2*vss)/g2, 0.0))
            sang = sqrt(max(0.25*(gs**2*vcc - 2*gc*gs*vcs + gc**2*vss)/g2**2, 0.0))/3.1415926535898*180
          end if
          write (64, '(3f10.4,6f12.6,f12.6,f12.6,2f10.3,i9)') gozd + (j - 1)*dvzd, goxd - (i - 1)*dvxd, depz(k), gc, &
            gstd(i, j, k, 1), gs, gstd(i, j, k, 2), gstdb(i, j, k, 1), gstdb(i, j, k, 2), amp, samp, fast_axis(gc, gs), sang, &
            nsamp(i, j)
        end do
      end do
    end do
    close (64)
  end if
  if (ngrp > 0) then   ! one block per wave type, in para.in's order; the lines end in the type's wavetp veltp
    open (64, file='noise_posterior_mc.dat')
    do g = 1, ngrp
      wavetp = p%seg_wavetp(g); veltp = p%seg_veltp(g)
      do j = 1, ny - 2
        do i = 1, nx - 2
          write (64, '(2f10.4,3f12.6,i6,2i3)') gozd + (j - 1)*dvzd, goxd - (i - 1)*dvxd, glam_mean(i, j, g), glam_std(i, j, g), &
            sigma_c*glam_mean(i, j, g), gndata(i, j, g), wavetp, veltp
        end do
      end do
    end do
    close (64)
  else if (noise_a0 > 0) then
    open (64, file='noise_posterior_mc.dat')
    do j = 1, ny - 2
      do i = 1, nx - 2
        write (64, '(2f10.4,3f12.6,i6)') gozd + (j - 1)*dvzd, goxd - (i - 1)*dvxd, lam_mean(i, j), lam_std(i, j), &
          sigma_c*lam_mean(i, j), ndata(i, j)
      end do
    end do
    close (64)
  end if
  if (prior_on .and. .not. noise_a0 > 0) then
    open (64, file='Vs_prior_check_mc.dat')
    do k = 1, nlay
      do j = 1, ny - 2
        do i = 1, nx - 2
          write (64, '(3f10.4,2f12.6,f12.5)') gozd + (j - 1)*dvzd, goxd - (i - 1)*dvxd, depz(k), std(i, j, k), res(i, j, k, 1), &
            ratio(i, j, k)
        end do
      end do
    end do
    close (64)
  end if
  open (78, file='cell_mc.dat')
  do j = 1, ny - 2
    do i = 1, nx - 2
      write (78, '(3f10.4,2f10.5)') gozd + (j - 1)*dvzd, goxd - (i - 1)*dvxd, acc(i, j), rms_b(i, j), rms_m(i, j)
    end do
  end do
  close (78)
  write (*, *) '  Program finishes successfully'
  write (66, *) '  Program finishes successfully'
  close (66)
  call dazim_finalize()

contains

  ! radial = 1: the chains on the stacked knots (Vsv, Vsh, deepest), their statistics, the log's summary and every file
  subroutine radial_run()
    integer :: n, kv, kh, nsv, nsh, a
    real :: couple, share
    real, allocatable :: vst(:, :, :), lo2(:, :, :), hi2(:, :, :), vmh(:, :, :), vbh(:, :, :)
    real, allocatable :: mean2(:, :, :), std2(:, :, :), qq2(:, :, :, :), best2(:, :, :), rhat2(:, :, :)
    real, allocatable, target :: xim(:, :, :), xis(:, :, :), xiq(:, :, :, :), xir(:, :, :), pg(:, :, :), cvh(:, :, :), vgm(:, :, :), &
                                 vgs(:, :, :)
    real*8, allocatable, target :: skv(:, :, :), skh(:, :, :)
    real, allocatable :: sd(:, :, :, :), cov(:, :, :), rd(:, :, :, :), rsm(:, :, :, :), cross(:, :, :, :), tr(:, :, :), rat(:, :, :, :)
    n = nlay
    kv = sum(p%type_kmax(1:2)); kh = sum(p%type_kmax(3:4))
    nsv = count(p%seg_wavetp(1:p%nseg) == 2); nsh = p%nseg - nsv
    couple = 0
    if (sigma_hv > 0) couple = 1/sigma_hv
    if (any(.not. (vmin > 0))) error stop 'radial = 1 needs a positive lower bound of Vs (Minvel, MOD - width)'
    allocate (vst(nx, ny, 2*n + 1), lo2(nx - 2, ny - 2, 2*n), hi2(nx - 2, ny - 2, 2*n))
    vst(:, :, 1:n) = vsf(:, :, 1:n); vst(:, :, n + 1:2*n) = vsf(:, :, 1:n); vst(:, :, 2*n + 1) = vsf(:, :, nz)
    lo2(:, :, 1:n) = vmin; lo2(:, :, n + 1:2*n) = vmin
    hi2(:, :, 1:n) = vmax; hi2(:, :, n + 1:2*n) = vmax
    call dazim_init(0)
    call dazim_check(dazim_mc_create(dazim_handle, nx, ny, 2*n + 1, kmax, nchain, nbin, seed, vst, lo2, hi2, cmap, wcov, step0, nadapt, &
                                     mc, nempty), 'Monte-Carlo chains')
    do q = 6, 66, 60
      write (q, '(a,i8,a,i8)') ' cells sampled', ncell - nempty, '  cells without data (start model kept)', nempty
    end do
    if (proposal /= 0) call dazim_check(dazim_mc_set_proposal(dazim_handle, mc, proposal), 'Monte-Carlo proposal')
    if (ntemp > 1) then
      allocate (beta(ntemp), swap_try(ntemp - 1, ncell - nempty), swap_acc(ntemp - 1, ncell - nempty))
      call dazim_check(dazim_mc_set_tempering(dazim_handle, mc, ntemp, tmax, nswap), 'Monte-Carlo tempering')
      call dazim_check(dazim_mc_temper_state(dazim_handle, mc, c_null_ptr, c_null_ptr, c_null_ptr, c_loc(beta), c_null_ptr, &
                                             c_null_ptr, c_null_ptr), 'tempering ladder')
      do q = 6, 66, 60
        write (q, '(a,64f8.3)') ' ladder, temperatures 1 / beta:', (1.0d0/beta(i), i=1, ntemp)
      end do
    end if
    call dazim_check(dazim_mc_set_segments(dazim_handle, mc, p%nseg, p%seg_wavetp, p%seg_veltp, p%seg_kmax), 'wave types')
    ngrp = 0
    if (noise_a0 > 0) then                      ! one noise scale per wave type, as without radial anisotropy
      ngrp = p%nseg
      allocate (grp(kmax))
      do g = 1, ngrp
        grp(sum(p%seg_kmax(1:g - 1)) + 1:sum(p%seg_kmax(1:g))) = g - 1
      end do
      ga0 = noise_a0; gb0 = noise_b0
      call dazim_check(dazim_mc_set_noise_groups(dazim_handle, mc, ngrp, grp, ga0, gb0), 'hierarchical noise per wave type')
    end if
    call dazim_check(dazim_mc_set_radial(dazim_handle, mc, couple), 'radial anisotropy')
    if (prior_on) call dazim_check(dazim_mc_set_prior(dazim_handle, mc, smooth_vs, damp_vs, c_null_ptr), 'Gaussian prior')
    call dazim_check(dazim_mc_run(dazim_handle, mc, depz, minthk, tRc, nsample, nsample, nnoroot), 'Monte-Carlo run')
    t_run = real(dazim_last_kernel_seconds(dazim_handle, 'mc'//c_null_char))
    t_disp = real(dazim_last_kernel_seconds(dazim_handle, 'mc.disp'//c_null_char))
    t_step = real(dazim_last_kernel_seconds(dazim_handle, 'mc.step'//c_null_char))
    ncov = nint(dazim_last_kernel_seconds(dazim_handle, 'mc.cov_cells'//c_null_char))
    allocate (mean2(nx - 2, ny - 2, 2*n), std2(nx - 2, ny - 2, 2*n), qq2(nx - 2, ny - 2, 2*n, 3), best2(nx - 2, ny - 2, 2*n))
    allocate (rhat2(nx - 2, ny - 2, 2*n), acc(nx - 2, ny - 2), chi2b(nx - 2, ny - 2))
    call dazim_check(dazim_mc_result(dazim_handle, mc, mean2, std2, qq2, best2, rhat2, acc, chi2b), 'posterior statistics')
    allocate (xim(nx - 2, ny - 2, n), xis(nx - 2, ny - 2, n), xiq(nx - 2, ny - 2, n, 3), xir(nx - 2, ny - 2, n), pg(nx - 2, ny - 2, n))
    allocate (cvh(nx - 2, ny - 2, n), vgm(nx - 2, ny - 2, n), vgs(nx - 2, ny - 2, n))
    call dazim_check(dazim_mc_radial_result(dazim_handle, mc, c_loc(xim), c_loc(xis), c_loc(xiq), c_loc(xir), c_loc(pg), c_loc(cvh), &
                                            c_loc(vgm), c_loc(vgs)), 'posterior statistics of xi')
    if (ntemp > 1) call dazim_check(dazim_mc_temper_state(dazim_handle, mc, c_null_ptr, c_null_ptr, c_null_ptr, c_null_ptr, &
                                                          c_null_ptr, c_loc(swap_try), c_loc(swap_acc)), 'swap counts')
    if (ngrp > 0) then
      allocate (glam_mean(nx - 2, ny - 2, ngrp), glam_std(nx - 2, ny - 2, ngrp), gndata(nx - 2, ny - 2, ngrp))
      call dazim_check(dazim_mc_noise_groups_result(dazim_handle, mc, glam_mean, glam_std, gndata), 'noise-scale posteriors')
    end if
    call dazim_check(dazim_mc_free(dazim_handle, mc), 'Monte-Carlo chains')

    ! ---- the curves of the mean and of the best models: the Rayleigh periods of Vsv, then the Love periods of Vsh ------------------
    allocate (vmc(nx, ny, nz), vmh(nx, ny, nz), vbest(nx, ny, nz), vbh(nx, ny, nz), pvm(nx*ny, kmax), pvb(nx*ny, kmax))
    vmc = vsf; vmh = vsf; vbest = vsf; vbh = vsf
    vmc(2:nx - 1, 2:ny - 1, 1:n) = mean2(:, :, 1:n); vmh(2:nx - 1, 2:ny - 1, 1:n) = mean2(:, :, n + 1:2*n)
    vbest(2:nx - 1, 2:ny - 1, 1:n) = best2(:, :, 1:n); vbh(2:nx - 1, 2:ny - 1, 1:n) = best2(:, :, n + 1:2*n)
    allocate (rms_b(nx - 2, ny - 2), rms_m(nx - 2, ny - 2), sampled(nx - 2, ny - 2))
    sampled = any(wcov /= 0.0, dim=3)
    call curves(vbest, vbh, pvb, .false.)
    if (prior_on .and. .not. noise_a0 > 0) then   ! the chains' stds against dazim_column_resolution_radial's at the mean models
      allocate (svs(nx*ny, max(kv, kh), nz), svp(nx*ny, max(kv, kh), nz), srho(nx*ny, max(kv, kh), nz))
      allocate (skv(nx*ny, kv, nz), skh(nx*ny, kh, nz))
      call curves(vmc, vmh, pvm, .true.)
      allocate (sd(nx - 2, ny - 2, n, 2), cov(nx - 2, ny - 2, n), rd(nx - 2, ny - 2, n, 2), rsm(nx - 2, ny - 2, n, 2))
      allocate (cross(nx - 2, ny - 2, n, 2), tr(nx - 2, ny - 2, 2), rat(nx - 2, ny - 2, n, 2))
      call dazim_check(dazim_column_resolution_radial(dazim_handle, nx, ny, n, kv, c_loc(skv), kh, c_loc(skh), wcov(:, :, 1:kv), &
                                                      wcov(:, :, kv + 1:kmax), smooth_vs, damp_vs, couple, sd, cov, rd, rsm, cross, tr, &
                                                      c_null_ptr, nempty_res, nbad), 'column resolution (Vsv, Vsh) at the mean models')
      rat = 0
      where (sd(:, :, :, 1) > 0) rat(:, :, :, 1) = std2(:, :, 1:n)/sd(:, :, :, 1)
      where (sd(:, :, :, 2) > 0) rat(:, :, :, 2) = std2(:, :, n + 1:2*n)/sd(:, :, :, 2)
    else
      call curves(vmc, vmh, pvm, .false.)
    end if
    s0 = 0; cnt = 0
    do j = 1, ny - 2
      do i = 1, nx - 2
        rms_b(i, j) = cell_rms(pvb, i, j)
        rms_m(i, j) = cell_rms(pvm, i, j)
        do t = 1, kmax
          if (wcov(i, j, t) /= 0.0) then
            s0 = s0 + (real(cmap(i, j, t), 8) - pvm(j*nx + i + 1, t))**2
            cnt = cnt + 1
          end if
        end do
      end do
    end do
    rms_all = 0
    if (cnt > 0) rms_all = real(sqrt(s0/cnt))

    ! ---- summary -----------------------------------------------------------------------------------------------------------------
    ns = count(sampled)
    do q = 6, 66, 60
      write (q, '(a,i12,a,i12)') ' proposals without a root:', nnoroot, ' of', int(2*nsample, 8)*ns*nchain
      write (q, '(a,f9.2,a,f9.2,a,f9.3,a)') ' run', t_run, ' s (dispersion calls', t_disp, ' s, step kernels', t_step, ' s)'
      if (proposal == 1) write (q, '(a,i8,a,i8)') ' cells with an adapted covariance:', ncov, ' of', ns
    end do
    if (ntemp > 1 .and. ns > 0) then
      nr = count(swap_try > 0)
      allocate (sorted(max(nr, 1)))
      sorted = 0
      if (nr > 0) sorted(1:nr) = pack(real(swap_acc)/real(max(swap_try, 1_c_int64_t)), swap_try > 0)
      call sort(sorted)
      do q = 6, 66, 60
        write (q, '(a,4f8.3)') ' swap acceptance over (cell, rung pair), minimum and quartiles 25/50/75 %:', sorted(1), &
          sorted(max(1, nint(0.25*nr))), sorted(max(1, nint(0.5*nr))), sorted(max(1, nint(0.75*nr)))
        write (q, '(a,i3,a,i3,a)') ' the statistics below are of the', ncold, ' chains per cell at T = 1 (of', nchain, ')'
      end do
      deallocate (sorted)
    end if
    if (ns > 0) then
      allocate (sorted(ns))
      sorted = pack(acc, sampled)
      call sort(sorted)
      do q = 6, 66, 60
        write (q, '(a,3f8.3)') ' acceptance over cells, quartiles 25/50/75 %:', sorted(max(1, nint(0.25*ns))), &
          sorted(max(1, nint(0.5*ns))), sorted(max(1, nint(0.75*ns)))
      end do
      deallocate (sorted)
      nr = count(spread(sampled, 3, 2*n) .and. rhat2 == rhat2)
      allocate (sorted(max(nr, 1)))
      sorted = 0
      if (nr > 0) sorted(1:nr) = pack(rhat2, spread(sampled, 3, 2*n) .and. rhat2 == rhat2)
      call sort(sorted)
      do q = 6, 66, 60
        write (q, '(a,2f9.4)') ' R-hat over (cell, Vsv and Vsh knot), median and maximum:', sorted(max(1, (nr + 1)/2)), sorted(max(nr, 1))
      end do
      deallocate (sorted)
      nr = count(spread(sampled, 3, n) .and. xir == xir)
      allocate (sorted(max(nr, 1)))
      sorted = 0
      if (nr > 0) sorted(1:nr) = pack(xir, spread(sampled, 3, n) .and. xir == xir)
      call sort(sorted)
      share = real(count(spread(sampled, 3, n) .and. (pg < 0.025 .or. pg > 0.975)))/real(ns*n)
      do q = 6, 66, 60
        write (q, '(a,2f9.4)') ' R-hat of xi over (cell, knot), median and maximum:', sorted(max(1, (nr + 1)/2)), sorted(max(nr, 1))
        write (q, '(a,f8.4)') ' share of sampled (cell, knot)s with P(xi > 1) outside [0.025, 0.975]:', share
      end do
      deallocate (sorted)
    end if
    do g = 1, p%nseg   ! per wave type: its periods, the mean |c residual| of the best models and, with the noise scales, the median lambda
      s0 = 0; cnt = 0
      do t = sum(p%seg_kmax(1:g - 1)) + 1, sum(p%seg_kmax(1:g))
        do j = 1, ny - 2
          do i = 1, nx - 2
            if (wcov(i, j, t) /= 0.0) then
              s0 = s0 + abs(real(cmap(i, j, t), 8) - pvb(j*nx + i + 1, t))
              cnt = cnt + 1
            end if
          end do
        end do
      end do
      if (cnt > 0) s0 = s0/cnt
      nr = 0
      if (ngrp > 0) nr = count(gndata(:, :, g) > 0 .and. glam_mean(:, :, g) == glam_mean(:, :, g))
      allocate (sorted(max(nr, 1)))
      sorted = 0
      if (nr > 0) sorted(1:nr) = pack(glam_mean(:, :, g), gndata(:, :, g) > 0 .and. glam_mean(:, :, g) == glam_mean(:, :, g))
      call sort(sorted)
      do q = 6, 66, 60
        if (ngrp > 0) then
          write (q, '(a,a,a,i3,a,f10.5,a,f9.3)') ' ', trim(type_name(p%seg_wavetp(g), p%seg_veltp(g))), ':', p%seg_kmax(g), &
            ' periods, best model mean |c residual| (km/s)', s0, ', median of the mean of lambda over cells', sorted(max(1, (nr + 1)/2))
        else
          write (q, '(a,a,a,i3,a,f10.5)') ' ', trim(type_name(p%seg_wavetp(g), p%seg_veltp(g))), ':', p%seg_kmax(g), &
            ' periods, best model mean |c residual| (km/s)', s0
        end if
      end do
      deallocate (sorted)
    end do
    if (prior_on .and. noise_a0 > 0) then
      do q = 6, 66, 60
        write (q, '(a)') ' Gaussian prior: Vsv_Vsh_prior_check_mc.dat is not written, with the noise scale unknown sigma_c is not the data std'
      end do
    else if (prior_on) then
      do a = 1, 2
        nr = count(spread(sampled, 3, n) .and. rat(:, :, :, a) > 0)
        allocate (sorted(max(nr, 1)))
        sorted = 0
        if (nr > 0) sorted(1:nr) = pack(rat(:, :, :, a), spread(sampled, 3, n) .and. rat(:, :, :, a) > 0)
        call sort(sorted)
        do q = 6, 66, 60
          write (q, '(a,a,a,3f9.4)') ' Gaussian prior: chains'' std / linearised std of ', merge('Vsv', 'Vsh', a == 1), &
            ' over (cell, knot), quartiles 25/50/75 %:', sorted(max(1, nint(0.25*nr))), sorted(max(1, (nr + 1)/2)), &
            sorted(max(1, nint(0.75*nr)))
        end do
        deallocate (sorted)
      end do
    end if
    do q = 6, 66, 60
      write (q, '(a,f12.5)') ' posterior-mean models: rms_c', rms_all
    end do

    ! ---- output files ------------------------------------------------------------------------------------------------------------
    call write_mod('MOD_mc', depz, vmc)
    call write_mod('MOD_Vsh_mc', depz, vmh)
    call write_vs_model('DSurfTomo_mc.inv', p, depz, vmc)
    call write_posterior('Vs_posterior_mc.dat', 0)
    call write_posterior('Vsh_posterior_mc.dat', n)
    open (64, file='xi_posterior_mc.dat')
    do k = 1, n
      do j = 1, ny - 2
        do i = 1, nx - 2
          write (64, '(3f10.4,5f10.5,f10.4,f9.4,f9.4,2f10.4)') gozd + (j - 1)*dvzd, goxd - (i - 1)*dvxd, depz(k), xim(i, j, k), &
            xis(i, j, k), xiq(i, j, k, 1), xiq(i, j, k, 2), xiq(i, j, k, 3), xir(i, j, k), pg(i, j, k), cvh(i, j, k), vgm(i, j, k), &
            vgs(i, j, k)
        end do
      end do
    end do
    close (64)
    call write_radial_model('Vsv_Vsh_model_mc.inv', p, depz, vmc, vmh, xim)
    call write_phase_map('period_phaseV_mc.dat', p, inner_cells(nx, ny, kmax, pvm))
    if (ngrp > 0) then
      open (64, file='noise_posterior_mc.dat')
      do g = 1, ngrp
        wavetp = p%seg_wavetp(g); veltp = p%seg_veltp(g)
        do j = 1, ny - 2
          do i = 1, nx - 2
            write (64, '(2f10.4,3f12.6,i6,2i3)') gozd + (j - 1)*dvzd, goxd - (i - 1)*dvxd, glam_mean(i, j, g), glam_std(i, j, g), &
              sigma_c*glam_mean(i, j, g), gndata(i, j, g), wavetp, veltp
          end do
        end do
      end do
      close (64)
    end if
    if (prior_on .and. .not. noise_a0 > 0) then
      open (64, file='Vsv_Vsh_prior_check_mc.dat')
      do k = 1, n
        do j = 1, ny - 2
          do i = 1, nx - 2
            write (64, '(3f10.4,2(2f12.6,f12.5))') gozd + (j - 1)*dvzd, goxd - (i - 1)*dvxd, depz(k), std2(i, j, k), sd(i, j, k, 1), &
              rat(i, j, k, 1), std2(i, j, n + k), sd(i, j, k, 2), rat(i, j, k, 2)
          end do
        end do
      end do
      close (64)
    end if
    open (78, file='cell_mc.dat')
    do j = 1, ny - 2
      do i = 1, nx - 2
        write (78, '(3f10.4,2f10.5)') gozd + (j - 1)*dvzd, goxd - (i - 1)*dvxd, acc(i, j), rms_b(i, j), rms_m(i, j)
      end do
    end do
    close (78)

  contains

    ! the Rayleigh curves of vv into pv(:, 1:kv) and the Love curves of vh into pv(:, kv+1:kmax); with kernels their dc/dVs tables
    subroutine curves(vv, vh, pv, kernels)
      real, intent(in) :: vv(:, :, :), vh(:, :, :)
      real*8, intent(out) :: pv(:, :)
      logical, intent(in) :: kernels
      type(c_ptr) :: ka, kb, kc
      ka = c_null_ptr; kb = c_null_ptr; kc = c_null_ptr
      if (kernels) then
        ka = c_loc(svs); kb = c_loc(svp); kc = c_loc(srho)
      end if
      call dazim_check(dazim_dispersion_kernels_typed(dazim_handle, nx, ny, nz, vv, depz, minthk, int(nsv, c_int), &
                                                      int(p%seg_wavetp(1:nsv), c_int), int(p%seg_veltp(1:nsv), c_int), &
                                                      int(p%seg_kmax(1:nsv), c_int), tRc(1:kv), pv(:, 1:kv), ka, kb, kc, nfail), &
                       'Rayleigh curves of Vsv')
      if (kernels) call dazim_check(dazim_vs_kernels(dazim_handle, nx, ny, nz, kv, vv, svs, svp, srho, skv), 'dc/dVsv table')
      call dazim_check(dazim_dispersion_kernels_typed(dazim_handle, nx, ny, nz, vh, depz, minthk, int(nsh, c_int), &
                                                      int(p%seg_wavetp(nsv + 1:p%nseg), c_int), int(p%seg_veltp(nsv + 1:p%nseg), c_int), &
                                                      int(p%seg_kmax(nsv + 1:p%nseg), c_int), tRc(kv + 1:kmax), pv(:, kv + 1:kmax), ka, &
                                                      kb, kc, nfail), 'Love curves of Vsh')
      if (kernels) call dazim_check(dazim_vs_kernels(dazim_handle, nx, ny, nz, kh, vh, svs, svp, srho, skh), 'dc/dVsh table')
    end subroutine

    ! Vs_posterior_mc.dat's lines for the knots k0 + 1 .. k0 + n of the stacked statistics
    subroutine write_posterior(fname, k0)
      character(len=*), intent(in) :: fname
      integer, intent(in) :: k0
      open (64, file=fname)
      do k = 1, n
        do j = 1, ny - 2
          do i = 1, nx - 2
            write (64, '(3f10.4,7f10.4)') gozd + (j - 1)*dvzd, goxd - (i - 1)*dvxd, depz(k), mean2(i, j, k0 + k), std2(i, j, k0 + k), &
              qq2(i, j, k0 + k, 1), qq2(i, j, k0 + k, 2), qq2(i, j, k0 + k, 3), best2(i, j, k0 + k), rhat2(i, j, k0 + k)
          end do
        end do
      end do
      close (64)
    end subroutine
  end subroutine

  ! RMS over the periods with a weight of cmap - c at inner cell (i1, j1); 0 for a cell without data
  real function cell_rms(pv, i1, j1)
    real*8, intent(in) :: pv(:, :)
    integer, intent(in) :: i1, j1
    integer :: t1, n1
    real*8 :: s
    s = 0; n1 = 0
    do t1 = 1, kmax
      if (wcov(i1, j1, t1) /= 0.0) then
        s = s + (real(cmap(i1, j1, t1), 8) - pv(j1*nx + i1 + 1, t1))**2
        n1 = n1 + 1
      end if
    end do
    cell_rms = 0
    if (n1 > 0) cell_rms = real(sqrt(s/n1))
  end function

  subroutine sort(a)   ! Shell sort with gaps 3h+1 (up to (nx-2)(ny-2)(nz-1) values)
    real, intent(inout) :: a(:)
    integer :: i1, j1, h
    real :: x
    h = 1
    do while (h < size(a)/3)
      h = 3*h + 1
    end do
    do while (h >= 1)
      do i1 = h + 1, size(a)
        x = a(i1)
        j1 = i1 - h
        do while (j1 >= 1)
          if (a(j1) <= x) exit
          a(j1 + h) = a(j1)
          j1 = j1 - h
        end do
        a(j1 + h) = x
      end do
      h = h/3
    end do
  end subroutine
end program
