! dazim_main.f90 -- DAzimSurfTomo_amd: the reference's inversion program (inv/Main_Jt.f90:1-835) with the hot
! path on one MI355X.  Same command line (`DAzimSurfTomo_amd para.in`), same input files (para.in, the
! traveltime data file, MOD) and the same output files (IterVel.out, MOD_Ref, DSurfTomo.inv, Gc_Gs_model.inv,
! period_phaseVMOD.dat, phaseV_FWD.dat, period_Azm_tomo.inv, Traveltime_statis_00th.dat, <para>_inv.log,
! lsmr.txt) in the reference's formats.
!
! What runs where, per outer iteration (inv/Main_Jt.f90:360-770):
!   device : dispersion + depth kernels, TI eigenfunction kernels (joint mode, dazim_ti_kernels), eikonal fields, rays + G rows
!            (dazim_assemble_G), residuals + CalDdatSigma weights + weighted right-hand side + row scaling (dazim_weight_data),
!            DWS (dazim_csr_col_abs_sums), the Tikhonov rows generated behind the ray rows (dazim_csr_append_tikhonov), LSMR
!            (dazim_lsmr_traced), the clamped model update and its statistics (dazim_model_update) and the G*dv diagnostics
!            (dazim_aprod on the resident un-thresholded rows).  G never leaves HBM; only O(m) + O(n) vectors cross PCIe.
!   host   : parsing, the O(n) copy of the regularisation stencil for the ||Lm|| diagnostics, formatted output.
! Joint (iso-mode F) inversions take the TI depth kernels Lsen_Gsc from ti_hip.f90 (the device kernels of ti.hip).
!
! `DAzimSurfTomo_amd para.in [uncertainty]`, uncertainty = 1 (default 0: nothing below is computed or written, and the program makes the
! calls and writes the bytes it does without the argument): how well the model is known, from dazim_model_posterior on the last outer
! iteration's [W G; L] (the matrix that iteration's LSMR was given, m_data = dall) with para.in's damping: the Tikhonov rows read as a
! Gaussian prior, the data errors as CalDdatSigma's sigma.  This is the exact regularised solution of the last linearised step; LSMR
! stopped at itnlim is an approximation to that solution, so the file describes what the step aims at, not LSMR's iterate.  One rank
! only: with DAZIM_NGPU > 1 the matrix is row-sharded and the program stops before the first iteration.
!   model_uncertainty.dat  lon lat depth, then std_post std_noise rdiag rsum width_h width_z of Vs (width_h in cells, width_z in km); in
!                          iso-mode F also std_post rdiag of Gc, std_post rdiag of Gs, and leak of Vs (the share of Vs's averaging
!                          kernel that lies in Gc, Gs); one line per inner cell and inverted knot in Vs_resolution_2step.dat's order
!   log + stdout: per knot trace(Rm) / ncell per block, the median std_post of Vs and (iso-mode F) the median leak of Vs; "not factored"
!                          when the normal matrix has no Cholesky factor
!
! `DAzimSurfTomo_amd para.in [uncertainty [tradeoff]]`, tradeoff = K >= 3 (default 0: as without the argument): on the same matrix and
! that iteration's right-hand side, dazim_model_tradeoff at the K factors 10^(-1 + 2k/(K-1)), k = 0 .. K-1, on weightVs and weightGcs
! together (sweep 1) and, in iso-mode F, on weightGcs alone with weightVs as given (sweep 2), with para.in's damping: the linearised
! step solved exactly at each factor.  The model the program inverts with is not changed.  One rank only, as uncertainty = 1.
!   tradeoff.dat           per point: sweep, factor, the effective weights per block and the damping, chi2, |L x|^2 per block (the rows
!                          at para.in's weights), |x|^2, the resolved parameters tr(Rm) per block, GCV, log evidence
!   log + stdout: per sweep the L-curve corner, the GCV minimum and the evidence maximum (dazim_tradeoff_pick)
program DAzimSurfTomo_amd
  use iso_c_binding
  use dazim_mod
  use dazim_io
  implicit none
  character(len=100) :: inputfile, logfile
  character(len=80) :: datafile
  type(para_t) :: p
  logical :: ex, iso_mod
  integer, allocatable :: dper(:)           ! virtual period of every datum (typed data: the type columns of Traveltime_statis)
  integer :: wavetp_i, veltp_i
  logical, external :: ti_kernels_on_device
  integer :: nx, ny, nz, nsrc, nrc, maxiter, kmaxRc, kmax
  real :: goxd, gozd, dvxd, dvzd, minthk, Minvel, Maxvel, spfra, weightVs, weightGcs, damp
  real*8, allocatable :: tRc(:), tRcV(:, :, :), pv(:, :)
  real, allocatable :: depz(:), vsf(:, :, :), gcf(:, :, :), gsf(:, :, :), Lsen_Gsc(:, :, :)
  real, allocatable :: scxf(:, :), sczf(:, :), rcxf(:, :, :), rczf(:, :, :)
  integer, allocatable :: periods(:, :), nrc1(:, :), nsrc1(:)
  real, allocatable :: obst(:), dist(:), dsyn(:), cbst(:), sigmaT(:), datweight(:), Tdata(:), resbst(:), fwdTvs(:), fwdTaa(:)
  real, allocatable :: dv(:), norm(:), yfull(:), xtmp(:), rwreg(:)
  integer, allocatable :: rowreg(:), colreg(:)
  integer :: dall, maxvp, maxm, iter, i, j, k, nar, nar1, nreg, count3, narVs, m, n, istop, itn, itnlim, localSize
  real :: mean, std_devs, meanAbs, meandeltaT, atol, btol, conlim, anorm, acond, rnorm, arnorm, xnorm, pertV
  real :: mindVs, maxdVs, meadVs, minGc, maxGc, meaGc, minGs, maxGs, meaGs, VariVs, VariGc, VariGs
  integer(8) :: maxnar
  type(c_ptr) :: G, Gd
  integer :: c0, c1, crate
  real :: wstats(8)
  real, allocatable :: ustats(:, :, :)       ! (3: min, max, sum |.| ; nz-1 ; block) of the update, from dazim_model_update
  integer(8) :: tk0, tk1, tkrate
  ! several GPUs (one process per GPU, dazim_ranks_init): this rank's contiguous share of the (period, source) fields -- its
  ! sources with their receivers (the *_l arrays, what the G assembly sees), its dloc data rows starting behind row d0 of the dall,
  ! its rows [treg0, treg1) of the regularisation block.  Everything the diagnostics and the output files read (dsyn, Tdata,
  ! datweight, fwdTvs, fwdTaa, the DWS) is put together over the ranks, so that every rank writes the same files.
  real, allocatable :: scxf_l(:, :), sczf_l(:, :), rcxf_l(:, :, :), rczf_l(:, :, :), dsyn_l(:)
  integer, allocatable :: periods_l(:, :), nrc1_l(:, :), nsrc1_l(:), wfield(:)
  integer :: nfield_all, f0, f1, fidx, d0, dloc, sl, treg0, treg1, nregblk
  real(8) :: tph(9) = 0                      ! wall seconds per phase, printed when DAZIM_TIMING is set (tools/run_test4_program.sh)
  character(len=8) :: timing_env
  ! uncertainty = 1
  integer :: iunc, ngpu_env, nblk_u
  integer(c_int) :: nbad
  character(len=32) :: ngpu_val
  real, allocatable, target :: upost(:, :), utrace(:, :), udepz(:)
  integer :: itrade                          ! tradeoff = K

  call system_clock(c0, crate)
  call system_clock(tk0, tkrate)
  open (36, file='lsmr.txt')
  write (*, *)
  write (*, *) '                       DAzimSurfTomo'
  write (*, *)
  if (command_argument_count() < 1) then                    ! inv/Main_Jt.f90:144-154
    write (*, *) 'input file [para.in (Default)]:'
    read (*, '(a)') inputfile
    if (len_trim(inputfile) <= 1) inputfile = 'para.in'
  else
    call get_command_argument(1, inputfile)
  end if
  inquire (file=inputfile, exist=ex)
  if (.not. ex) stop 'unable to open the inputfile'
  iunc = 0
  if (command_argument_count() >= 2) call optional_arg(2, iunc)
  itrade = 0
  if (command_argument_count() >= 3) call optional_arg(3, itrade)
  if (itrade /= 0 .and. itrade < 3) then
    write (*, '(a,i6)') ' ERROR: tradeoff is 0 or the number of sweep points, at least 3; it is', itrade
    error stop 'bad tradeoff argument'
  end if
  if (iunc == 1 .or. itrade > 0) then         ! (before any rank is started)
    ngpu_env = 1
    call get_environment_variable('DAZIM_NGPU', ngpu_val)
    if (len_trim(ngpu_val) > 0) read (ngpu_val, *) ngpu_env
    if (ngpu_env > 1 .and. iunc == 1) then
      write (*, '(a)') ' ERROR: uncertainty = 1 needs the whole matrix on one GPU; with DAZIM_NGPU > 1 its rows are sharded over the ranks'
      error stop 'uncertainty = 1 with more than one rank'
    else if (ngpu_env > 1) then
      write (*, '(a)') ' ERROR: tradeoff > 0 needs the whole matrix on one GPU; with DAZIM_NGPU > 1 its rows are sharded over the ranks'
      error stop 'tradeoff > 0 with more than one rank'
    end if
  end if

  ! ---- para.in, inv/Main_Jt.f90:158-214 -------------------------------------------------------------
  call read_para(inputfile, p)
  datafile = p%datafile; nx = p%nx; ny = p%ny; nz = p%nz; goxd = p%goxd; gozd = p%gozd; dvxd = p%dvxd; dvzd = p%dvzd
  minthk = p%minthk; Minvel = p%Minvel; Maxvel = p%Maxvel; nsrc = p%nsrc; spfra = p%spfra; maxiter = p%maxiter; iso_mod = p%iso_mod
  weightVs = p%weightVs; weightGcs = p%weightGcs; damp = p%damp; kmaxRc = p%kmaxRc; tRc = p%tRc
  write (*, *) 'input Rayleigh wave phase velocity data file:'
  write (*, '(a)') datafile
  write (*, *) 'model origin:latitude,longitue'
  write (*, '(2f10.4)') goxd, gozd
  write (*, *) 'grid spacing:latitude,longitue'
  write (*, '(2f10.4)') dvxd, dvzd
  write (*, *) 'model dimension:nx,ny,nz'
  write (*, '(3i5)') nx, ny, nz
  write (*, *) 'depth refined interval layer '
  write (*, '(f8.1)') minthk
  write (*, *) 'smoothing for dVsv '
  write (*, '(f8.1)') weightVs
  write (*, *) 'smoothing for Gc, Gs '
  write (*, '(f8.1)') weightGcs
  write (*, *) 'damping'
  write (*, '(f8.1)') damp
  if (nz <= 1) stop 'error nz value.'
  write (*, *) 'number of period'
  write (*, '(i6)') kmaxRc
  if (kmaxRc <= 0) stop 'Can only deal with Rayleigh wave phase velocity data!'
  if (p%typed .and. .not. iso_mod) then
    write (*, '(a)') ' ERROR: DAzimSurfTomo_amd, joint mode (iso_mod = F): para.in lists Rayleigh group or Love-wave periods; the 2-psi'
    write (*, '(a)') ' depth kernels (Lsen_Gsc) exist for Rayleigh phase velocities only.  Invert such data in iso mode (iso_mod = T).'
    stop 'joint mode takes Rayleigh phase velocities only'
  end if
  if (p%typed) call dazim_set_segments(p%nseg, p%seg_wavetp, p%seg_veltp, p%seg_kmax)
  write (logfile, '(a,a)') trim(inputfile), '_inv.log'
  open (66, file=logfile)
  write (66, *)
  write (66, *) '                  DAzimSurfTomo'
  write (66, *)
  write (66, *) 'model origin:latitude,longitue'
  write (66, '(2f10.4)') goxd, gozd
  write (66, *) 'grid spacing:latitude,longitue'
  write (66, '(2f10.4)') dvxd, dvzd
  write (66, *) 'model dimension:nx,ny,nz'
  write (66, '(3i5)') nx, ny, nz
  write (*, *) 'Rayleigh wave phase velocity used,periods:(s)'
  write (*, '(50f6.1)') (tRc(i), i=1, kmaxRc)
  write (66, *) 'Rayleigh wave phase velocity used,periods:(s)'
  write (66, '(50f6.1)') (tRc(i), i=1, kmaxRc)
  nrc = nsrc
  kmax = kmaxRc

  ! ---- traveltime data file, inv/Main_Jt.f90:240-318 -------------------------------------------------
  call read_data(p, scxf, sczf, rcxf, rczf, periods, nrc1, nsrc1, obst, dist, dall, dper)

  maxvp = (nx - 2)*(ny - 2)*(nz - 1)
  maxnar = int(spfra*real(dall)*real(nx)*real(ny)*real(nz)*3.0, 8)     ! sparsity fraction, inv/Main_Jt.f90:324
  allocate (dv(3*maxvp), norm(maxvp), cbst(dall + 3*maxvp), dsyn(dall))
  allocate (sigmaT(dall), datweight(dall), Tdata(dall), resbst(dall), fwdTvs(dall), fwdTaa(dall))
  allocate (Lsen_Gsc(nx*ny, kmaxRc, nz - 1), gcf(nx - 2, ny - 2, nz - 1), gsf(nx - 2, ny - 2, nz - 1))
  allocate (tRcV(nx - 2, ny - 2, kmaxRc), pv(nx*ny, kmaxRc))
  allocate (yfull(dall + 3*maxvp), xtmp(3*maxvp), rwreg(7*3*maxvp), rowreg(7*3*maxvp), colreg(7*3*maxvp))
  gcf = 0; gsf = 0; Lsen_Gsc = 0

  ! ---- initial model, inv/Main_Jt.f90:346-356 -----------------------------------------------------------
  call read_mod('MOD', p, depz, vsf)
  write (*, *) ' grid points in depth direction:(km)'
  write (*, '(50f7.2)') depz

  allocate (ustats(3, nz - 1, 3))
  call tick(1)                               ! inputs read
  call dazim_ranks_init()
  ! ---- this rank's share of the fields (all of them with one rank) ----
  nfield_all = sum(nsrc1(1:kmax))
  allocate (wfield(max(nfield_all, 1)))
  fidx = 0
  do k = 1, kmax
    do i = 1, nsrc1(k)
      fidx = fidx + 1
      wfield(fidx) = nrc1(i, k)
    end do
  end do
  call dazim_shard_fields(nfield_all, wfield, dazim_nranks, dazim_rank, f0, f1)
  allocate (scxf_l(nsrc, kmax), sczf_l(nsrc, kmax), rcxf_l(nrc, nsrc, kmax), rczf_l(nrc, nsrc, kmax))
  allocate (periods_l(nsrc, kmax), nrc1_l(nsrc, kmax), nsrc1_l(kmax))
  scxf_l = 0; sczf_l = 0; rcxf_l = 0; rczf_l = 0; periods_l = 0; nrc1_l = 0; nsrc1_l = 0
  fidx = 0; d0 = 0; dloc = 0
  do k = 1, kmax
    do i = 1, nsrc1(k)
      if (fidx >= f0 .and. fidx < f1) then
        nsrc1_l(k) = nsrc1_l(k) + 1
        sl = nsrc1_l(k)
        scxf_l(sl, k) = scxf(i, k); sczf_l(sl, k) = sczf(i, k)
        rcxf_l(:, sl, k) = rcxf(:, i, k); rczf_l(:, sl, k) = rczf(:, i, k)
        periods_l(sl, k) = periods(i, k); nrc1_l(sl, k) = nrc1(i, k)
        dloc = dloc + nrc1(i, k)
      else if (fidx < f0) then
        d0 = d0 + nrc1(i, k)
      end if
      fidx = fidx + 1
    end do
  end do
  ! (a decision every rank takes together: one that stopped on its own would leave the others waiting in their next collective)
  if (dazim_allmax_int(merge(1, 0, dloc < 1)) > 0) then
    call dazim_finalize()
    stop 'a rank has no data: more ranks than (period, source) fields'
  end if
  allocate (dsyn_l(dloc))
  if (dazim_nranks > 1) write (*, '(a,i3,a,i3,a,i8,a,i8,a,i8)') '  rank ', dazim_rank, ' of ', dazim_nranks, ': fields ', f0 + 1, ' ..', f1, &
    ', data rows ', dloc
  call tick(2)                               ! HIP context
  open (34, file='IterVel.out')
  do iter = 1, maxiter
    write (6, *) ' -----------------------------------------------------------'
    write (66, *) ' -----------------------------------------------------------'
    if (iso_mod) then
      write (66, *) iter, 'th iteration, invert for isotropic Vs para.'
      write (6, *) iter, 'th iteration, invert for isotropic Vs para.'
      maxm = maxvp
    else
      write (66, *) iter, 'th iteration, invert for dVs, Gc, Gs '
      write (6, *) iter, 'th iteration, invert for dVs, Gc, Gs '
      maxm = maxvp*3
    end if
    write (6, *) ' -----------------------------------------------------------'
    write (66, *) ' -----------------------------------------------------------'

    ! ---- forward problem + sensitivity matrix on the device (CalSurfG / CalSurfGAnisoJoint) ---------------
    dsyn = 0; tRcV = 0
    if (.not. iso_mod .and. .not. ti_kernels_on_device()) &
      call ti_depth_kernels(nx, ny, nz, vsf, kmaxRc, tRc, depz, minthk, Lsen_Gsc)
    ! The reference keeps every ray row twice: the triplets rw/iw/col with |row| > ftol for the solver (inv/CalSurfG.f90:1358)
    ! and the dense GVs/GGc/GGs for the residual diagnostics (inv/CalSigamNorm.f90:73), which hold EVERY entry of the cells with
    ! |fdm| >= ftol, the dVs block with the Brocher derivatives left over from the last such cell (:1369-1378).  Option
    ! rays.dense_twin makes the library build that second matrix from the same cell lists: Gd, resident, never scaled.
    call dazim_check(dazim_set_option(dazim_handle, 'rays.dense_twin'//c_null_char, 1_c_int), 'option')
    call dazim_assemble_G(.not. iso_mod, nx, ny, nz, vsf, dsyn_l, Lsen_Gsc, goxd, gozd, dvxd, dvzd, kmaxRc, tRc, periods_l, depz, &
                          minthk, scxf_l, sczf_l, rcxf_l, rczf_l, nrc1_l, nsrc1_l, kmax, nsrc, nrc, G, nar, pv, &
                          ti_here=(.not. iso_mod .and. ti_kernels_on_device()))
    dsyn(d0 + 1:d0 + dloc) = dsyn_l(1:dloc)   ! (dsyn = 0 above: the other ranks' predicted times arrive with the sum)
    call dazim_allsum(dsyn, dall)
    call dazim_check(dazim_set_option(dazim_handle, 'rays.dense_twin'//c_null_char, 0_c_int), 'option')
    call dazim_check(dazim_csr_take_twin(dazim_handle, G, Gd), 'dense twin')
    ! inv/CalSurfGAniso_Joint.f90:801-811 (the iso branch leaves tRcV = 0)
    if (.not. iso_mod) tRcV = inner_cells(nx, ny, kmaxRc, pv)
    call tick(3)                             ! dispersion + eikonal + rays + G on the device
    if (iter == 1) call write_phase_map('period_phaseVMOD.dat', p, tRcV)
    call tick(9)

    ! ---- residuals, CalDdatSigma weights, weighted right-hand side and row scaling on the device, inv/Main_Jt.f90:432-470 ----
    cbst = 0                                  ! (the rows of the regularisation block keep a zero right-hand side)
    if (dazim_nranks > 1) then
      Tdata = 0; datweight = 0
    end if
    call dazim_check(dazim_weight_data_sharded(dazim_handle, G, int(dloc, c_int64_t), int(d0, c_int64_t), int(dall, c_int64_t), &
                                               obst(d0 + 1:), dsyn(d0 + 1:), Tdata(d0 + 1:), datweight(d0 + 1:), cbst, wstats), &
                     'data weights')
    call dazim_allsum(Tdata, dall)
    call dazim_allsum(datweight, dall)
    meandeltaT = wstats(5)
    write (6, '(a, f12.4,a,f10.2,a,f10.2,a)') '  Before Inversion: abs mean, std, RMS of Res:', wstats(3), ' s ', &
      wstats(2), ' s ', wstats(4), ' s'
    write (66, '(a, f12.4,a,f10.2,a,f10.2,a)') '  Before Inversion: abs mean, std, RMS of Res:', wstats(3), ' s ', &
      wstats(2), ' s ', wstats(4), ' s'
    write (6, '(a, f8.3, a, f8.3,a, f7.3, a)') '  mean data weight:', wstats(7), &
      ' |  abs data mean with weight:', wstats(8), 's  |  dt/t0:', meandeltaT*100, ' %'
    write (66, '(a, f8.3, a, f8.3,a, f7.3, a)') '  mean data weight:', wstats(7), &
      ' |  abs data mean with weight:', wstats(8), 's  |  dt/t0:', meandeltaT*100, ' %'
    if (iso_mod) then
      call dazim_check(dazim_csr_col_abs_sums(dazim_handle, G, norm), 'DWS')   ! inv/Main_Jt.f90:477-481
      call dazim_allsum(norm, maxvp)
    end if

    call tick(4)                             ! residuals, weights, row scaling, DWS
    ! ---- regularisation rows appended to the resident matrix, inv/Main_Jt.f90:483-500 ----------------------------
    nar1 = nar
    if (iter == 1) then                       ! the rows depend on the grid and the weights only: the host copy (used by the ||Lm||
      nreg = 0; count3 = 0; narVs = 0         ! diagnostics) is made once, the matrix block is generated on the device every time
      call laplacian_rows(0, weightVs)
      if (.not. iso_mod) then
        narVs = nreg
        call laplacian_rows(1, weightGcs)
        call laplacian_rows(2, weightGcs)
      end if
    end if
    nar = nar1 + nreg
    ! inv/Main_Jt.f90:523 tests the whole system's entries: the ranks' ray rows summed + the regularisation block, the same number
    ! and hence the same decision on every rank
    if (dazim_allsum_int8(int(nar1, 8)) + nreg > maxnar) then
      call dazim_finalize()
      stop 'increase sparsity fraction(spfra)'
    end if
    nregblk = merge(1, 3, iso_mod)
    call dazim_shard_rows(nregblk*maxvp, dazim_nranks, dazim_rank, treg0, treg1)   ! (all of them with one rank)
    if (iso_mod) then
      call dazim_check(dazim_csr_append_tikhonov_rows(dazim_handle, G, nx, ny, nz, 1_c_int, [weightVs], int(treg0, c_int64_t), &
                                                      int(treg1, c_int64_t)), 'Tikhonov rows')
    else
      call dazim_check(dazim_csr_append_tikhonov_rows(dazim_handle, G, nx, ny, nz, 3_c_int, [weightVs, weightGcs, weightGcs], &
                                                      int(treg0, c_int64_t), int(treg1, c_int64_t)), 'Tikhonov rows')
    end if
    write (*, '(a,3f8.2)') '  damp,  lamebda Gsc, lamebda Vs: ', damp, weightGcs, weightVs
    write (66, '(a,3f8.2)') '  damp,  lamebda Gsc, lamebda Vs: ', damp, weightGcs, weightVs
    m = dall + count3
    n = maxm
    if (p%typed) then                         ! (typed data only: the log of Rayleigh phase input keeps its bytes)
      write (6, '(a,i9,a,i9,a,i12)') '  [G; L] rows m =', m, '  unknowns n =', n, '  entries nnz =', dazim_allsum_int8(int(nar1, 8)) + nreg
      write (66, '(a,i9,a,i9,a,i12)') '  [G; L] rows m =', m, '  unknowns n =', n, '  entries nnz =', dazim_allsum_int8(int(nar1, 8)) + nreg
    end if

    call tick(5)                             ! Tikhonov rows
    ! ---- LSMR on the device, inv/Main_Jt.f90:534-574 ----------------------------------------------------------------
    dv = 0
    if (iso_mod) then
      atol = 1e-3; btol = 1e-3; conlim = 1200; itnlim = 1000; localSize = n/4
    else
      atol = 1e-5; btol = 1e-4; conlim = 200; itnlim = 500; localSize = 10
    end if
    block                                     ! lsmr.txt carries the reference's iteration log (nout = 36, inv/Main_Jt.f90:136,562)
      type(dazim_lsmr_rec), allocatable :: tr(:)
      integer(c_int) :: ntr
      allocate (tr(itnlim + 2))
      call dazim_check(dazim_lsmr_traced(dazim_handle, G, cbst, damp, atol, btol, conlim, itnlim, localSize, dv, istop, itn, &
                                         anorm, acond, rnorm, arnorm, xnorm, tr, int(itnlim + 2, c_int), ntr), 'LSMR')
      call dazim_lsmr_log(36, m, n, damp, atol, btol, conlim, itnlim, localSize, tr, int(ntr), istop, itn, anorm, acond, rnorm, &
                          arnorm, xnorm)
    end block
    if (istop == 3) then
      write (*, '(a)') '  istop = 3, large condition number, LSMR failed'
      write (66, '(a)') '  istop = 3, large condition number, LSMR failed'
    end if
    write (*, '(a)') '  Finish LSMR.......'
    write (*, '(a, i7)') '  itn=               ', itn
    write (66, '(a, i7)') '  itn=               ', itn
    write (*, '(a, f7.1)') '  L2 norm of A=      ', anorm
    write (*, '(a, f7.1)') '  Condition NO. of A=', acond
    write (66, '(a, f7.1)') '  Condition NO. of A=', acond
    write (*, '(a, f7.1)') '  rnorm=             ', rnorm
    write (*, '(a, f7.1)') '  arnorm=            ', arnorm
    write (*, '(a, f7.3)') '  norm of dv =       ', xnorm

    call tick(6)                             ! LSMR + its log
    ! ---- clamped model update, inv/Main_Jt.f90:576-618 ------------------------------------------------------------------
    if (.not. iso_mod) then
      gcf = 0; gsf = 0
    end if
    call dazim_check(dazim_model_update(dazim_handle, nx, ny, nz, merge(0_c_int, 1_c_int, iso_mod), vsf, dv, Minvel, Maxvel, &
                                        gcf, gsf, ustats), 'model update')

    ! ---- statistics of the update, inv/Main_Jt.f90:621-666 (min, max, sum |.| per block and depth from the device) ----------
    mindVs = minval(ustats(1, :, 1)); maxdVs = maxval(ustats(2, :, 1)); meadVs = sum(ustats(3, :, 1))/maxvp
    write (6, '(a,3f10.4)') '  min  max and abs mean  dVs (km/s)', mindVs, maxdVs, meadVs
    write (66, '(a,3f10.4)') '  min  max and abs mean  dVs (km/s)', mindVs, maxdVs, meadVs
    if (.not. iso_mod) then
      minGc = minval(ustats(1, :, 2))*100; maxGc = maxval(ustats(2, :, 2))*100; meaGc = sum(ustats(3, :, 2))/maxvp*100
      minGs = minval(ustats(1, :, 3))*100; maxGs = maxval(ustats(2, :, 3))*100; meaGs = sum(ustats(3, :, 3))/maxvp*100
      write (6, '(a,3f10.4)') '  min  max and abs mean   Gc/L (%) ', minGc, maxGc, meaGc
      write (66, '(a,3f10.4)') '  min  max and abs mean   Gc/L (%) ', minGc, maxGc, meaGc
      write (6, '(a,3f10.4)') '  min  max and abs mean   Gs/L (%) ', minGs, maxGs, meaGs
      write (66, '(a,3f10.4)') '  min  max and abs mean   Gs/L (%) ', minGs, maxGs, meaGs
    end if
    do k = 1, nz - 1
      VariVs = ustats(3, k, 1)/((nx - 2)*(ny - 2))
      if (iso_mod) then
        write (66, '(a,f5.1,a,f5.1,a,f10.4)') '  Z ', depz(k), ' - ', depz(k + 1), ' km  abs mean dVs (km/s)', VariVs
        write (6, '(a,f5.1,a,f5.1,a,f10.4)') '  Z ', depz(k), ' - ', depz(k + 1), ' km  abs mean dVs (km/s)', VariVs
      else
        VariGc = ustats(3, k, 2)/((nx - 2)*(ny - 2))
        VariGs = ustats(3, k, 3)/((nx - 2)*(ny - 2))
        write (66, '(a, f5.1, a, f5.1, a, 2f10.3, f9.4)') '  Z ', depz(k), ' - ', depz(k + 1), &
          ' km  Abs Mean Gc (%)  Gs (%)   dVs (km/s)', VariGc*100, VariGs*100, VariVs
        write (6, '(a, f5.1, a, f5.1, a, 2f10.3, f9.4)') '  Z ', depz(k), ' - ', depz(k + 1), &
          ' km  Abs Mean Gc (%)  Gs (%)   dVs (km/s)', VariGc*100, VariGs*100, VariVs
      end if
    end do

    call tick(7)                             ! update + statistics
    ! ---- model-norm and residual diagnostics (Calmodel2Norm*, Cal*ReslNorm*, inv/CalSigamNorm.f90) -----------------------
    call model_norms()
    call residual_norms()
    call tick(8)                             ! G*dv diagnostics
    if (iter == 1 .or. iter == maxiter) then            ! inv/Main_Jt.f90:701-718 (id stays '00' in the reference)
      open (88, file='Traveltime_statis_00th.dat')
      if (iso_mod) then
        if (p%typed) then                     ! two trailing columns: wavetp veltp
          write (88, '(7a)') '   Dist(km)   T_obs(s)  T_ref_iso   Res(in)   dT(dvs)   Res(out) wavetp veltp'
          do i = 1, dall
            call period_type(p, dper(i), wavetp_i, veltp_i)
            write (88, '(3f10.3, 3e12.3, 2i3)') dist(i), obst(i), dsyn(i), Tdata(i), fwdTvs(i), resbst(i), wavetp_i, veltp_i
          end do
        else
        write (88, '(7a)') '   Dist(km)   T_obs(s)  T_ref_iso   Res(in)   dT(dvs)   Res(out)'
        do i = 1, dall
          write (88, '(3f10.3, 3e12.3)') dist(i), obst(i), dsyn(i), Tdata(i), fwdTvs(i), resbst(i)
        end do
        end if
      else
        write (88, '(7a)') '          Dist(km)       T_obs(s)        T_ref-iso        Res(in)   ', &
          'dT(aa)        dT(dvs)        Res(out)'
        do i = 1, dall
          write (88, '(3f10.4, 4e12.3)') dist(i), obst(i), dsyn(i), Tdata(i), fwdTvs(i), fwdTaa(i), resbst(i)
        end do
      end if
      close (88)
    end if
    mean = sum(resbst(1:dall))/dall
    meanAbs = sum(abs(resbst(1:dall)))/dall
    std_devs = sqrt(sum((resbst(1:dall) - mean)**2)/dall)
    write (6, '(a,f12.4,a,f10.2,a,f10.2,a)') '  After Inversion: abs mean, std, RMS of Res :', meanAbs, ' s ', &
      std_devs, ' s ', nrm2(dall, resbst)/sqrt(real(dall)), ' s'
    write (66, '(a,f12.4,a,f10.2,a,f10.2,a)') '  After Inversion: abs mean, std, RMS of Res :', meanAbs, ' s ', &
      std_devs, ' s ', nrm2(dall, resbst)/sqrt(real(dall)), ' s'

    if (iso_mod) then                                     ! inv/Main_Jt.f90:731-746
      write (34, *) ',OUTPUT S VELOCITY AT ITERATION', iter
      do k = 1, nz
        do j = 1, ny
          write (34, '(100f7.3)') (vsf(i, j, k), i=1, nx)
        end do
      end do
      write (34, *) ',OUTPUT DWS AT ITERATION', iter
      do k = 1, nz - 1
        do j = 2, ny - 1
          write (34, '(100f10.3)') (norm((k - 1)*(ny - 2)*(nx - 2) + (j - 2)*(nx - 2) + i - 1), i=2, nx - 1)
        end do
      end do
    end if
    write (66, '(a)') ' '
    write (6, '(a)') '  '
    if (iunc == 1 .and. iter == maxiter) then   ! on this iteration's [W G; L], before it is freed
      nblk_u = merge(1, 3, iso_mod)
      allocate (upost(nblk_u*maxvp, 7), utrace(nz - 1, nblk_u), udepz(nz - 1))
      upost = 0; utrace = 0
      udepz = depz(1:nz - 1)
      call dazim_check(dazim_model_posterior(dazim_handle, G, int(dall, c_int64_t), nx, ny, nz, merge(0_c_int, 1_c_int, iso_mod), damp, &
                                             c_loc(udepz), upost(:, 1), upost(:, 2), upost(:, 3), upost(:, 4), c_loc(upost(:, 5)), &
                                             c_loc(upost(:, 6)), merge(c_null_ptr, c_loc(upost(:, 7)), iso_mod), 0_c_int, c_null_ptr, &
                                             c_null_ptr, c_loc(utrace), nbad), 'model posterior')
    end if
    if (itrade > 0 .and. iter == maxiter) call tradeoff_sweeps()
    call dazim_check(dazim_csr_free(dazim_handle, G), 'free G')
    call dazim_check(dazim_csr_free(dazim_handle, Gd), 'free Gd')
    call tick(9)                             ! output files of the iteration
  end do

  ! ---- final models, inv/Main_Jt.f90:751-790 ---------------------------------------------------------------------------------
  call write_mod('MOD_Ref', depz, vsf)
  call write_vs_model('DSurfTomo.inv', p, depz, vsf)
  call write_azimuthal('Gc_Gs_model.inv', p, depz, vsf, gcf, gsf)
  call write_phase_map('phaseV_FWD.dat', p, tRcV)
  write (*, '(a)') '  Begin forward calculate period azimuthal A1, A2.'
  call write_period_azimuthal('period_Azm_tomo.inv', p, Lsen_Gsc, gcf, gsf, tRcV)
  if (iunc == 1 .and. allocated(upost)) &   ! (nbad > 0: the one matrix was not factored, so no depth is)
    call write_uncertainty('model_uncertainty.dat', p, 'dazim_model_posterior', 'depth', real(depz(1:nz - 1), 8), 'Vs Gc Gs', 6, upost, utrace, &
                           int(nbad), .false.)
  write (66, *) '  -----------------------------------------------------------'
  write (*, *) '  Program finishes successfully'
  write (66, *) '  Program finishes successfully'
  write (*, *) '  Output inverted shear velocity model: Vs_model_Syn.rela  Vs_model_Syn.abs'
  write (66, *) '  Output inverted shear velocity model: Vs_model_Syn.rela  Vs_model_Syn.abs'
  call tick(9)
  call get_environment_variable('DAZIM_TIMING', timing_env)
  if (len_trim(timing_env) > 0) then
    write (0, '(a,9f8.3)') ' phase seconds: read init assemble weights tikhonov lsmr update diag output ', tph
    ! (with several ranks the first three are this rank's block of the model, the last two its share of the fields)
    write (0, '(a,i3,a,5f8.3)') ' rank ', dazim_rank, ' device seconds: curves copies ti eikonal rays ', dazim_dev_seconds
  end if
  call system_clock(c1)
  write (*, '(a, f13.1, a)') '   All time cost= ', real(c1 - c0)/real(crate), "s"
  write (66, '(a, f13.1, a)') '   All time cost= ', real(c1 - c0)/real(crate), "s"
  close (36); close (66); close (34)
  call dazim_finalize()

contains

  subroutine tick(i)                         ! wall time since the previous tick goes to phase i
    integer, intent(in) :: i
    call system_clock(tk1)
    tph(i) = tph(i) + real(tk1 - tk0, 8)/real(tkrate, 8)
    tk0 = tk1
  end subroutine

  ! tradeoff.dat and the log's lines: dazim_model_tradeoff on this iteration's [W G; L] and weighted right-hand side cbst (the
  ! regularisation rows of G hold para.in's weights, so the sweep's scale is the factor itself), before the matrix is freed.  The
  ! sweeps are the points of ONE call, sweep after sweep, so the Gram matrix of the data rows is formed once for both.
  subroutine tradeoff_sweeps()
    integer :: nb, nsw, npt, s, k1, p0, p1
    integer(c_int) :: corner, igcv, iev
    real, allocatable :: tscale(:, :), tdamp(:), tw(:)
    real(c_double), allocatable :: tchi2(:), treg2(:, :), txn(:), tlda(:), tldp(:), tdof(:, :), tgcv(:), tlev(:), tsum(:)
    integer(c_int), allocatable :: tbad(:)
    nb = merge(1, 3, iso_mod)
    nsw = merge(1, 2, iso_mod)
    npt = nsw*itrade
    allocate (tscale(nb, npt), tdamp(npt), tw(nb), tchi2(npt), treg2(nb, npt), txn(npt), tlda(npt), tldp(npt), tdof(nb, npt), tgcv(npt), &
              tlev(npt), tsum(npt), tbad(npt))
    tw(1) = weightVs
    if (nb == 3) tw(2:3) = weightGcs
    tdamp = damp
    do s = 1, nsw
      do k1 = 1, itrade
        tscale(:, (s - 1)*itrade + k1) = tradeoff_factor(k1, itrade)
        if (s == 2) tscale(1, itrade + k1) = 1.0
      end do
    end do
    call dazim_check(dazim_model_tradeoff(dazim_handle, G, int(dall, c_int64_t), cbst, nx, ny, nz, merge(0_c_int, 1_c_int, iso_mod), &
                                          int(npt, c_int), tscale, tdamp, 1_c_int, 1_c_int, tchi2, treg2, txn, tlda, tldp, tdof, tgcv, &
                                          tlev, c_null_ptr, tbad), 'model tradeoff')
    tsum = sum(treg2, dim=1)
    open (45, file='tradeoff.dat', status='replace', action='write')
    do s = 1, nsw
      p0 = (s - 1)*itrade + 1; p1 = s*itrade
      call dazim_check(dazim_tradeoff_pick(int(itrade, c_int), tchi2(p0:p1), tsum(p0:p1), tgcv(p0:p1), tlev(p0:p1), corner, igcv, iev), &
                       'tradeoff pick')
      call write_tradeoff(45, 66, s, trim(merge('all blocks', 'Gc and Gs ', s == 1)), itrade, nb, tw, tscale(:, p0:p1), tdamp(p0:p1), &
                          tchi2(p0:p1), treg2(:, p0:p1), txn(p0:p1), tdof(:, p0:p1), tgcv(p0:p1), tlev(p0:p1), int(corner), int(igcv), &
                          int(iev))
    end do
    close (45)
  end subroutine

  ! scaled 2-norm like the reference's dnrm2 (inv/lsmrblas.f90:247)
  real function nrm2(nn, x)
    integer, intent(in) :: nn
    real, intent(in) :: x(*)
    real :: scale, ssq, absxi
    integer :: ix
    scale = 0.0; ssq = 1.0
    do ix = 1, nn
      if (x(ix) /= 0.0) then
        absxi = abs(x(ix))
        if (scale < absxi) then
          ssq = 1.0 + ssq*(scale/absxi)**2
          scale = absxi
        else
          ssq = ssq + (absxi/scale)**2
        end if
      end if
    end do
    nrm2 = scale*sqrt(ssq)
  end function

  ! first-order Tikhonov rows of one column block: 7-point Laplacian (6,-1 x6) inside, a lone 2 on the faces;
  ! inv/TikhRegul.f90:2 (iso) and :108 (joint: blocks dVs | Gc | Gs).  Appends to rowreg/colreg/rwreg.
  subroutine laplacian_rows(blk, weight)
    integer, intent(in) :: blk
    real, intent(in) :: weight
    integer :: nvx, nvz, ic, jc, kc, c, off(6), q
    nvx = nx - 2; nvz = ny - 2
    off = [-1, 1, -nvx, nvx, -nvz*nvx, nvz*nvx]
    do kc = 1, nz - 1
      do jc = 1, nvz
        do ic = 1, nvx
          count3 = count3 + 1
          c = (kc - 1)*nvz*nvx + (jc - 1)*nvx + ic + blk*maxvp
          if (ic == 1 .or. ic == nvx .or. jc == 1 .or. jc == nvz .or. kc == 1 .or. kc == nz - 1) then
            nreg = nreg + 1
            rowreg(nreg) = dall + count3; colreg(nreg) = c; rwreg(nreg) = 2.0*weight
          else
            nreg = nreg + 1
            rowreg(nreg) = dall + count3; colreg(nreg) = c; rwreg(nreg) = 6.0*weight
            do q = 1, 6
              nreg = nreg + 1
              rowreg(nreg) = dall + count3; colreg(nreg) = c + off(q); rwreg(nreg) = -1.0*weight
            end do
          end if
        end do
      end do
    end do
  end subroutine

  ! ||Lm|| over the regularisation entries exactly as the reference forms it (entry-wise products rw*dv(col), not
  ! row sums); inv/CalSigamNorm.f90:226 (iso) and :285 (joint)
  subroutine model_norms()
    real, allocatable :: Lm(:), LmW(:)
    integer :: q
    allocate (Lm(nreg), LmW(nreg))
    if (iso_mod) then
      do q = 1, nreg
        LmW(q) = rwreg(q)*dv(colreg(q))
        Lm(q) = LmW(q)/weightVs
      end do
      write (6, '(a,2f12.3)') '  dVs:  ||Lm||^2      and ||wLm||^2    : ', nrm2(nreg, Lm), nrm2(nreg, LmW)
      write (66, '(a,2f12.3)') '  dVs:  ||Lm||^2      and ||wLm||^2    : ', nrm2(nreg, Lm), nrm2(nreg, LmW)
    else
      do q = 1, nreg
        LmW(q) = rwreg(q)*dv(colreg(q))
        if (q <= narVs) then
          Lm(q) = LmW(q)/weightVs
        else
          Lm(q) = LmW(q)/weightGcs
        end if
      end do
      write (6, '(a,2f12.3)') '  dVs:  ||Lm||^2   and   ||wLm||^2     : ', nrm2(narVs, Lm), nrm2(narVs, LmW)
      write (66, '(a,2f12.3)') '  dVs:  ||Lm||^2   and   ||wLm||^2     : ', nrm2(narVs, Lm), nrm2(narVs, LmW)
      write (6, '(a,2f12.3)') '  Gcs:  ||Lm||^2   and   ||wLm||^2     : ', nrm2(nreg - narVs, Lm(narVs + 1:)), &
        nrm2(nreg - narVs, LmW(narVs + 1:))
      write (66, '(a,2f12.3)') '  Gcs:  ||Lm||^2   and   ||wLm||^2     : ', nrm2(nreg - narVs, Lm(narVs + 1:)), &
        nrm2(nreg - narVs, LmW(narVs + 1:))
      write (6, '(a,2f12.3)') '  All:  ||Lm||^2   and   ||wLm||^2     : ', nrm2(nreg, Lm), nrm2(nreg, LmW)
      write (66, '(a,2f12.3)') '  All:  ||Lm||^2   and   ||wLm||^2     : ', nrm2(nreg, Lm), nrm2(nreg, LmW)
      write (66, '(a)') '  '
      write (6, '(a)') '  '
    end if
  end subroutine

  ! predicted traveltime changes: the reference's dense matmul(GVs, dv) (+ GGc, GGs), inv/CalSigamNorm.f90:44 (iso) and :154
  ! (joint), as products with the resident un-thresholded, un-weighted rows Gd (= the entries GVs/GGc/GGs hold)
  subroutine residual_norms()
    real, allocatable :: resW(:)
    integer :: q
    real :: mabs
    allocate (resW(dall))
    xtmp(1:n) = 0; xtmp(1:maxvp) = dv(1:maxvp)
    yfull(1:dloc) = 0                         ! (Gd holds this rank's data rows; the sum over the ranks puts the vector together)
    call dazim_check(dazim_aprod(dazim_handle, 1, Gd, xtmp, yfull), 'aprod')
    fwdTvs = 0
    fwdTvs(d0 + 1:d0 + dloc) = yfull(1:dloc)
    call dazim_allsum(fwdTvs, dall)
    fwdTaa = 0
    if (.not. iso_mod) then
      xtmp(1:n) = dv(1:n); xtmp(1:maxvp) = 0
      yfull(1:dloc) = 0
      call dazim_check(dazim_aprod(dazim_handle, 1, Gd, xtmp, yfull), 'aprod')
      fwdTaa(d0 + 1:d0 + dloc) = yfull(1:dloc)
      call dazim_allsum(fwdTaa, dall)
    end if
    do q = 1, dall
      resbst(q) = Tdata(q) - fwdTaa(q) - fwdTvs(q)
      resW(q) = resbst(q)*datweight(q)
    end do
    if (iso_mod) then
      write (6, '(a,2f12.3)') '  dVs:  ||(Gm-d)||^2  and ||W(Gm-d)||^2: ', nrm2(dall, resbst), nrm2(dall, resW)
      write (66, '(a,2f12.3)') '  dVs:  ||(Gm-d)||^2  and ||W(Gm-d)||^2: ', nrm2(dall, resbst), nrm2(dall, resW)
    else
      write (6, '(a,2f12.3)') '  All:  ||(Gm-d)||^2  and ||W(Gm-d)||^2: ', nrm2(dall, resbst), nrm2(dall, resW)
      write (66, '(a,2f12.3)') '  All:  ||(Gm-d)||^2  and ||W(Gm-d)||^2: ', nrm2(dall, resbst), nrm2(dall, resW)
      write (66, '(a)') '  '
      write (6, '(a)') '  '
      mabs = sum(abs(fwdTaa(1:dall)))/dall
      write (66, '(a,f12.4,a)') '  ABS Mean T(AA): ', mabs, 's'
      write (6, '(a,f12.4,a)') '  ABS Mean T(AA): ', mabs, 's'
      mabs = sum(abs(fwdTvs(1:dall)))/dall
      write (66, '(a,f12.4,a)') '  ABS Mean T(dVs):', mabs, 's'
      write (6, '(a,f12.4,a)') '  ABS Mean T(dVs):', mabs, 's'
    end if
  end subroutine
end program
