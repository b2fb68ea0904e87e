! dazim_depth.f90 -- SurfDepthFromMaps_amd: the second step of the classical two-step method.  It turns the per-period maps of
! SurfPhaseMaps_amd into a depth model, cell by cell, on one MI355X: Vs(z) from each cell's phase-velocity dispersion curve and, in
! iso-mode F, Gc/L(z) and Gs/L(z) from its 2-psi curves (DESIGN.md section 13).
!
!   SurfDepthFromMaps_amd para.in [smooth_vs [smooth_gcs [sigma_c [resolution [map_sigma [radial [sigma_hv]]]]]]]
!
! Inputs: the unchanged para.in and MOD of DAzimSurfTomo_amd (read_para, read_mod of module dazim_io; the data file is not opened),
! the maps period_phaseV_map.dat (and period_Azm_tomo_map.inv in iso-mode F) and, if present, period_map_coverage.dat.  Weights:
! 1/sigma_c (default 0.01 km/s) where the map's DWS > 0, 0 elsewhere (everywhere 1/sigma_c without a coverage file).  smooth_vs /
! smooth_gcs default to para.in's two smoothing weights; the damping is para.in's.
! Vs: para.in's maxiter linearised iterations from MOD, each dazim_dispersion_kernels -> dazim_vs_kernels -> r = c_map - pvRc on the
! inner cells (w = 0 where pvRc = 0) -> dazim_column_lsq (nlay = nz-1) -> dazim_model_update (para.in's minvel, maxvel).
! Gc, Gs (iso-mode F): on the final Vs, dazim_ti_kernels, then one dazim_column_lsq on Lsen_Gsc with the two right-hand sides a1, a2:
! the 2-psi terms are linear in Gc, Gs, so they are solved for whole.
! map_sigma = 1 (default 0): the Vs weights become 1/max(sigma_c, std_post) per cell and period where DWS > 0, std_post the posterior
! std of c in period_map_uncertainty.dat (SurfPhaseMaps_amd with uncertainty = 1; the run stops without that file); sigma_c is then a
! floor, and a std that is not finite means no data.
! resolution = 1 (default 0: nothing below is computed or written): how well the answer is known, per inner cell and inverted knot,
! from dazim_column_resolution on the final model: one more dazim_dispersion_kernels with kernels, dazim_vs_kernels, then the
! posterior std (the regulariser read as a Gaussian prior), the std that the data errors 1/w alone leave, the diagonal and the row
! sum of the resolution matrix and the depth spread of its row, with the Vs solve's weights, smoothing and damping; in iso-mode F
! the same on Lsen_Gsc with smooth_gcs (Gc and Gs share K, so they share the numbers).  These are the statistics of the last
! linearised step: the regulariser acts on the update, not on the model.
! radial = 1 (default 0: everything above, unchanged): radial anisotropy (DESIGN.md section 13.1).  Vsv from the Rayleigh maps and Vsh
! from the Love maps of each cell, each through the isotropic code on its own column (Vp and rho of a column from that column's Vs
! by the Brocher relations; the weak cross-sensitivities Rayleigh to Vsh and Love to Vsv are neglected), tied by a Gaussian prior on
! Vsh - Vsv of std sigma_hv km/s (default 0.2; 0 = no coupling).  para.in must list Rayleigh and Love periods and iso-mode T.  Both
! profiles start from MOD and keep its deepest knot.  Each iteration: dazim_dispersion_kernels_typed with the Rayleigh segments on
! Vsv and with the Love segments on Vsh, dazim_vs_kernels on each, residuals and weights per virtual period as above, one
! dazim_column_lsq_radial with couple = 1 / sigma_hv and d0 = Vsh - Vsv, dazim_model_update on each profile.  resolution = 1 then
! calls dazim_column_resolution_radial with kernels at the final model.
!
! Outputs (names distinct from the other programs' so that all three can share a directory; formats of DAzimSurfTomo_amd's files):
!   DSurfTomo_2step.inv        as DSurfTomo.inv                MOD_2step     as MOD_Ref (a MOD for DAzimSurfTomo_amd)
!   period_phaseV_2step.dat    c of the final model, as period_phaseV_map.dat
!   Gc_Gs_model_2step.inv, period_Azm_tomo_2step.inv   (iso-mode F) as Gc_Gs_model.inv, period_Azm_tomo.inv
!   <para>_2step.log + stdout  one line per iteration: cells used, RMS c misfit before and predicted after the solve, max |dVs|
!   Vs_resolution_2step.dat    (resolution = 1) lon lat depth Vs std_post std_noise rdiag rsum width, one line per inner cell and
!                              inverted knot in DSurfTomo_2step.inv's order
!   Gc_Gs_resolution_2step.dat (resolution = 1, iso-mode F) the same without the Vs column
!   radial = 1: MOD_2step and DSurfTomo_2step.inv hold Vsv, period_phaseV_2step.dat the Rayleigh periods of Vsv and the Love periods of
!   Vsh, the log line the Rayleigh and the Love misfit side by side, and there are
!   MOD_Vsh_2step                 as MOD_2step, Vsh
!   Vsv_Vsh_model_2step.inv       lon lat depth Vsv Vsh Voigt-Vs xi on the whole grid, Voigt-Vs = sqrt((2 Vsv^2 + Vsh^2) / 3), xi = (Vsh / Vsv)^2
!   Vsv_Vsh_resolution_2step.dat  (resolution = 1) lon lat depth Vsv Vsh xi std_vsv std_vsh corr std_xi rdiag_v rdiag_h cross_v cross_h per
!                                 inner cell and inverted knot; std_xi = 2 xi sqrt(max(0, (std_vsh / Vsh)^2 + (std_vsv / Vsv)^2 - 2 cov / (Vsv Vsh)))
program SurfDepthFromMaps_amd
  use iso_c_binding
  use dazim_mod
  use dazim_io
  implicit none
  character(len=100) :: inputfile, logfile
  type(para_t) :: p
  logical :: ex, iso_mod
  integer :: nx, ny, nz, maxiter, kmax
  real :: minthk, Minvel, Maxvel, damp, smooth_vs, smooth_gcs, sigma_c
  real*8, allocatable :: tRc(:)
  real, allocatable :: depz(:), vsf(:, :, :)
  real*8, allocatable, target :: pv(:, :), svs(:, :, :), svp(:, :, :), srho(:, :, :), skern(:, :, :)
  real, allocatable, target :: lsen(:, :, :)
  real, allocatable :: cmap(:, :, :), amap(:, :, :, :), wcov(:, :, :), w(:, :, :), r(:, :, :, :), x(:, :, :, :)
  real, allocatable :: gcf(:, :, :), gsf(:, :, :), ustats(:, :), stats(:, :, :), res(:, :, :, :), rtrace(:, :)
  real*8, allocatable :: pvk(:, :)
  integer :: ires, isig, irad, kv, kh, nsv, nsh
  real :: sigma_hv
  real, allocatable :: vsh(:, :, :)
  real*8, allocatable, target :: skv(:, :, :), skh(:, :, :)
  integer(c_int) :: nbad
  real :: dummy1(1), rms0, rms1, maxdv
  real*8 :: s0, s1, cnt
  integer :: i, t, iter, nlay, nused, col, q
  integer(c_int) :: nfail, nempty

  write (*, *)
  write (*, *) '                       SurfDepthFromMaps'
  write (*, *)
  if (command_argument_count() < 1) error stop 'usage: SurfDepthFromMaps_amd para.in [smooth_vs [smooth_gcs [sigma_c [resolution [map_sigma [radial [sigma_hv]]]]]]]'
  call get_command_argument(1, inputfile)
  inquire (file=inputfile, exist=ex)
  if (.not. ex) error stop 'unable to open the inputfile'
  call read_para(inputfile, p)
  nx = p%nx; ny = p%ny; nz = p%nz; minthk = p%minthk; Minvel = p%Minvel; Maxvel = p%Maxvel; maxiter = p%maxiter
  iso_mod = p%iso_mod; damp = p%damp; kmax = p%kmaxRc; tRc = p%tRc
  if (nz <= 1) error stop 'error nz value.'
  if (kmax <= 0) error stop 'Can only deal with Rayleigh wave phase velocity data!'
  smooth_vs = p%weightVs; smooth_gcs = p%weightGcs; sigma_c = 0.01
  call optional_arg(2, smooth_vs)
  call optional_arg(3, smooth_gcs)
  call optional_arg(4, sigma_c)
  if (sigma_c <= 0) error stop 'sigma_c must be positive'
  ires = 0
  call optional_arg(5, ires)
  if (ires /= 0 .and. ires /= 1) then
    write (*, '(a,i0)') ' ERROR: resolution must be 0 or 1, not ', ires
    error stop 'bad argument'
  end if
  isig = 0
  call optional_arg(6, isig)
  if (isig /= 0 .and. isig /= 1) then
    write (*, '(a,i0)') ' ERROR: map_sigma must be 0 or 1, not ', isig
    error stop 'bad argument'
  end if
  irad = 0
  call optional_arg(7, irad)
  if (irad /= 0 .and. irad /= 1) then
    write (*, '(a,i0)') ' ERROR: radial must be 0 or 1, not ', irad
    error stop 'bad argument'
  end if
  sigma_hv = 0.2
  call optional_arg(8, sigma_hv)
  if (sigma_hv < 0) error stop 'sigma_hv must not be negative'
  if (irad == 1) then
    if (sum(p%type_kmax(3:4)) == 0) then
      write (*, '(a)') ' ERROR: radial = 1: para.in lists no Love periods (kmaxLc, kmaxLg); Vsh is what the Love maps constrain.'
      error stop 'radial = 1 needs Love periods'
    end if
    if (sum(p%type_kmax(1:2)) == 0) then
      write (*, '(a)') ' ERROR: radial = 1: para.in lists no Rayleigh periods (kmaxRc, kmaxRg); Vsv is what the Rayleigh maps constrain.'
      error stop 'radial = 1 needs Rayleigh periods'
    end if
    if (.not. iso_mod) then
      write (*, '(a)') ' ERROR: radial = 1 with iso-mode F: Gc/Gs together with radial anisotropy is not supported.  Run with iso-mode T.'
      error stop 'radial = 1 needs iso-mode T'
    end if
  end if
  nlay = nz - 1
  if (nlay > 63) error stop 'SurfDepthFromMaps_amd inverts at most 63 layers (nz <= 64)'
  if (kmax > 60) then
    write (*, '(a,i4,a)') ' ERROR: SurfDepthFromMaps_amd: para.in lists', kmax, ' periods over all wave types; the column solve holds at most 60'
    error stop 'SurfDepthFromMaps_amd takes at most 60 periods'
  end if
  if (p%typed .and. .not. iso_mod) then
    write (*, '(a)') ' ERROR: SurfDepthFromMaps_amd with iso_mod = F: para.in lists Rayleigh group or Love-wave periods; the Gc/Gs solve''s'
    write (*, '(a)') ' kernels (Lsen_Gsc) exist for Rayleigh phase velocities only.  Run such maps with iso_mod = T.'
    error stop 'the Gc/Gs solve takes Rayleigh phase velocities only'
  end if
  if (p%typed) call dazim_set_segments(p%nseg, p%seg_wavetp, p%seg_veltp, p%seg_kmax)
  write (logfile, '(a,a)') trim(inputfile), '_2step.log'
  open (66, file=logfile)
  write (66, *)
  write (66, *) '                  SurfDepthFromMaps'
  write (66, *)
  do q = 6, 66, 60
    write (q, '(a,3i5,a,i3,a,i3,a,l2)') ' grid nx ny nz:', nx, ny, nz, ';', kmax, ' periods; iterations', maxiter, '; iso-mode', iso_mod
    write (q, '(a,50f6.1)') ' periods (s):', (tRc(i), i=1, kmax)
    write (q, '(a,2f8.3,a,f8.3,a,f8.4,a,2f8.3)') ' smoothing Vs, Gc/Gs:', smooth_vs, smooth_gcs, '  damping', damp, &
      '  sigma_c (km/s)', sigma_c, '  Vs range', Minvel, Maxvel
  end do

  call read_mod('MOD', p, depz, vsf)

  ! ---- the maps ------------------------------------------------------------------------------------------------------------------
  allocate (cmap(nx - 2, ny - 2, kmax), wcov(nx - 2, ny - 2, kmax))
  call read_map('period_phaseV_map.dat', p, 4, 4, cmap, .true.)
  call coverage_weights(p, sigma_c, wcov)
  if (isig == 1) call uncertainty_weights(p, sigma_c, wcov)
  if (.not. iso_mod) then
    allocate (amap(nx - 2, ny - 2, kmax, 2))
    call read_map('period_Azm_tomo_map.inv', p, 9, 8, amap(:, :, :, 1), .true.)
    call read_map('period_Azm_tomo_map.inv', p, 9, 9, amap(:, :, :, 2), .false.)
  end if

  if (irad == 1) then
    call radial_inversion()
  else
    ! ---- Vs, para.in's iterations from MOD -----------------------------------------------------------------------------------------
    call dazim_init(0)
    allocate (pv(nx*ny, kmax), svs(nx*ny, kmax, nz), svp(nx*ny, kmax, nz), srho(nx*ny, kmax, nz), skern(nx*ny, kmax, nz))
    allocate (w(nx - 2, ny - 2, kmax), r(nx - 2, ny - 2, kmax, 2), x(nx - 2, ny - 2, nlay, 2), ustats(3, nlay), stats(2, kmax, 2))
    do q = 6, 66, 60
      write (q, '(a)') '  iter  cells  rms_c_before  rms_c_after   max|dVs|'
    end do
    do iter = 1, maxiter
      call dazim_check(dazim_dispersion_any(dazim_handle, nx, ny, nz, vsf, depz, minthk, kmax, tRc, pv, c_loc(svs), c_loc(svp), &
                                                c_loc(srho), nfail), 'dispersion and depth kernels')
      if (nfail > 0) write (6, *) 'WARNING:improper initial value in disper - no zero found', nfail
      call dazim_check(dazim_vs_kernels(dazim_handle, nx, ny, nz, kmax, vsf, svs, svp, srho, skern), 'dc/dVs table')
      call residual()
      call dazim_check(dazim_column_lsq(dazim_handle, nx, ny, nlay, kmax, 0, c_loc(skern), 1, r, w, smooth_vs, damp, x, nempty, &
                                        stats), 'column solve (Vs)')
      s1 = 0
      do t = 1, kmax
        s1 = s1 + real(stats(2, t, 1), 8)**2*count(w(:, :, t) > 0.0)
      end do
      rms1 = 0
      if (cnt > 0) rms1 = real(sqrt(s1/cnt))
      call dazim_check(dazim_model_update(dazim_handle, nx, ny, nz, 0, vsf, x, Minvel, Maxvel, dummy1, dummy1, ustats), 'model update')
      maxdv = maxval(abs(x(:, :, :, 1)))
      do q = 6, 66, 60
        write (q, '(i6,i7,2f14.5,f11.4)') iter, nused, rms0, rms1, maxdv
      end do
    end do

    ! ---- the final model's curves; its misfit --------------------------------------------------------------------------------------
    call dazim_check(dazim_dispersion_any(dazim_handle, nx, ny, nz, vsf, depz, minthk, kmax, tRc, pv, c_null_ptr, c_null_ptr, &
                                              c_null_ptr, nfail), 'dispersion curves of the final model')
    call residual()
    do q = 6, 66, 60
      write (q, '(a,i7,a,f12.5)') ' final model: cells', nused, '  rms_c', rms0
    end do

    ! ---- how well that Vs is known (resolution = 1): kernels at the final model, the last solve's weights and regularisers ----------
    if (ires == 1) then
      allocate (res(nx - 2, ny - 2, nlay, 5), rtrace(nx - 2, ny - 2), pvk(nx*ny, kmax))
      call dazim_check(dazim_dispersion_any(dazim_handle, nx, ny, nz, vsf, depz, minthk, kmax, tRc, pvk, c_loc(svs), c_loc(svp), &
                                                c_loc(srho), nfail), 'depth kernels of the final model')
      call dazim_check(dazim_vs_kernels(dazim_handle, nx, ny, nz, kmax, vsf, svs, svp, srho, skern), 'dc/dVs table of the final model')
      call dazim_check(dazim_column_resolution(dazim_handle, nx, ny, nlay, kmax, 0, c_loc(skern), w, smooth_vs, damp, depz, &
                                               res(:, :, :, 1), res(:, :, :, 2), res(:, :, :, 3), res(:, :, :, 4), res(:, :, :, 5), &
                                               c_null_ptr, rtrace, nempty, nbad), 'column resolution (Vs)')
      call write_resolution('Vs_resolution_2step.dat', p, depz, res, vsf)
      do q = 6, 66, 60
        write (q, '(a)') ' resolution: posterior std and resolution matrix of the last linearised step (the regulariser acts on the update)'
      end do
      call resolution_log('Vs   ')
    end if

    ! ---- Gc, Gs on the final Vs (iso-mode F) ---------------------------------------------------------------------------------------
    if (.not. iso_mod) then
      allocate (lsen(nx*ny, kmax, nz - 1), gcf(nx - 2, ny - 2, nlay), gsf(nx - 2, ny - 2, nlay))
      call dazim_check(dazim_ti_kernels(dazim_handle, nx, ny, nz, vsf, depz, minthk, kmax, tRc, pv, lsen), 'TI depth kernels')
      r = amap
      call dazim_check(dazim_column_lsq(dazim_handle, nx, ny, nlay, kmax, 1, c_loc(lsen), 2, r, w, smooth_gcs, damp, x, nempty, &
                                        stats), 'column solve (Gc, Gs)')
      gcf = x(:, :, :, 1); gsf = x(:, :, :, 2)
      do q = 6, 66, 60
        write (q, '(a,2f12.6,a,2f12.6)') ' Gc/Gs: rms a1, a2', sqrt(sum(stats(1, :, 1)**2)/kmax), sqrt(sum(stats(1, :, 2)**2)/kmax), &
          '  rms misfit a1, a2', sqrt(sum(stats(2, :, 1)**2)/kmax), sqrt(sum(stats(2, :, 2)**2)/kmax)
        write (q, '(a,2f10.5)') ' max |Gc|, |Gs|:', maxval(abs(gcf)), maxval(abs(gsf))
      end do
      if (ires == 1) then
        call dazim_check(dazim_column_resolution(dazim_handle, nx, ny, nlay, kmax, 1, c_loc(lsen), w, smooth_gcs, damp, depz, &
                                                 res(:, :, :, 1), res(:, :, :, 2), res(:, :, :, 3), res(:, :, :, 4), res(:, :, :, 5), &
                                                 c_null_ptr, rtrace, nempty, nbad), 'column resolution (Gc, Gs)')
        call write_resolution('Gc_Gs_resolution_2step.dat', p, depz, res)
        call resolution_log('Gc/Gs')
      end if
    end if

    ! ---- output files, in the formats of DAzimSurfTomo_amd's (dazim_main.f90) --------------------------------------------------------
    call write_mod('MOD_2step', depz, vsf)
    call write_vs_model('DSurfTomo_2step.inv', p, depz, vsf)
    call write_phase_map('period_phaseV_2step.dat', p, inner_cells(nx, ny, kmax, pv))
    if (.not. iso_mod) then
      call write_azimuthal('Gc_Gs_model_2step.inv', p, depz, vsf, gcf, gsf)
      call write_period_azimuthal('period_Azm_tomo_2step.inv', p, lsen, gcf, gsf, inner_cells(nx, ny, kmax, pv))
    end if
  end if
  write (*, *) '  Program finishes successfully'
  write (66, *) '  Program finishes successfully'
  close (66)
  call dazim_finalize()

contains

  ! one log line of a dazim_column_resolution call: the cells it used, and the median and the minimum over them of trace(R) / nlay,
  ! the share of the cell's knots that the data resolve
  subroutine resolution_log(what)
    character(len=*), intent(in) :: what
    real, allocatable :: s(:)
    real :: v
    integer :: m, gap, i1, j1
    s = pack(rtrace, any(w /= 0.0, dim=3))/nlay
    m = size(s)
    gap = m/2
    do while (gap > 0)                              ! Shell sort
      do i1 = gap + 1, m
        v = s(i1); j1 = i1
        do while (j1 > gap)
          if (s(j1 - gap) <= v) exit
          s(j1) = s(j1 - gap); j1 = j1 - gap
        end do
        s(j1) = v
      end do
      gap = gap/2
    end do
    do q = 6, 66, 60
      if (m > 0) then
        write (q, '(a,a,a,i7,a,i5,a,2f9.5)') ' resolution ', what, ': cells', m, '  not factored', nbad, &
          '  trace(R)/nlay median, min', s((m + 1)/2), s(1)
      else
        write (q, '(a,a,a,i7)') ' resolution ', what, ': cells', m
      end if
    end do
  end subroutine

  ! radial = 1: Vsv (vsf) from the Rayleigh periods, the leading kv virtual periods, and Vsh from the kh Love periods after them
  subroutine radial_inversion()
    real :: couple, rmsv0, rmsh0, rmsv1, rmsh1
    real, allocatable :: d0(:, :, :), sd(:, :, :, :), cov(:, :, :), rd(:, :, :, :), rsum(:, :, :, :), cross(:, :, :, :), tr(:, :, :)
    kv = sum(p%type_kmax(1:2)); kh = sum(p%type_kmax(3:4))
    nsv = count(p%seg_wavetp(1:p%nseg) == 2); nsh = p%nseg - nsv
    couple = 0
    if (sigma_hv > 0) couple = 1/sigma_hv
    vsh = vsf
    call dazim_init(0)
    ! (svs, svp, srho serve both wave types in turn, as the flat [nz][kv | kh][nx*ny] tables the calls fill and read)
    allocate (pv(nx*ny, kmax), svs(nx*ny, max(kv, kh), nz), svp(nx*ny, max(kv, kh), nz), srho(nx*ny, max(kv, kh), nz))
    allocate (skv(nx*ny, kv, nz), skh(nx*ny, kh, nz), d0(nx - 2, ny - 2, nlay))
    allocate (w(nx - 2, ny - 2, kmax), r(nx - 2, ny - 2, kmax, 1), x(nx - 2, ny - 2, nlay, 2), ustats(3, nlay), stats(2, kmax, 1))
    do q = 6, 66, 60
      write (q, '(a,i3,a,i3,a,f8.4,a,f9.4)') ' radial anisotropy:', kv, ' Rayleigh periods (Vsv),', kh, ' Love periods (Vsh); sigma_hv (km/s)', &
        sigma_hv, '  coupling', couple
      write (q, '(a)') '  iter  cells  rms_c_before  rms_c_after  rms_R_before  rms_L_before   rms_R_after   rms_L_after  max|dVsv|  max|dVsh|'
    end do
    do iter = 1, maxiter
      call tables(.true.)
      call residual()
      rmsv0 = rms_of(1, kv); rmsh0 = rms_of(kv + 1, kmax)
      d0 = vsh(2:nx - 1, 2:ny - 1, 1:nlay) - vsf(2:nx - 1, 2:ny - 1, 1:nlay)
      call dazim_check(dazim_column_lsq_radial(dazim_handle, nx, ny, nlay, kv, c_loc(skv), kh, c_loc(skh), r(:, :, 1:kv, 1), &
                                               r(:, :, kv + 1:kmax, 1), w(:, :, 1:kv), w(:, :, kv + 1:kmax), d0, smooth_vs, damp, couple, x, &
                                               nempty, stats), 'column solve (Vsv, Vsh)')
      rmsv1 = after(1, kv); rmsh1 = after(kv + 1, kmax); rms1 = after(1, kmax)
      call dazim_check(dazim_model_update(dazim_handle, nx, ny, nz, 0, vsf, x(:, :, :, 1), Minvel, Maxvel, dummy1, dummy1, ustats), &
                       'model update (Vsv)')
      call dazim_check(dazim_model_update(dazim_handle, nx, ny, nz, 0, vsh, x(:, :, :, 2), Minvel, Maxvel, dummy1, dummy1, ustats), &
                       'model update (Vsh)')
      do q = 6, 66, 60
        write (q, '(i6,i7,6f14.5,2f11.4)') iter, nused, rms0, rms1, rmsv0, rmsh0, rmsv1, rmsh1, maxval(abs(x(:, :, :, 1))), &
          maxval(abs(x(:, :, :, 2)))
      end do
    end do
    ! the final models' curves and their misfit; with resolution = 1 from the kernels' call
    call tables(ires == 1)
    call residual()
    rmsv0 = rms_of(1, kv); rmsh0 = rms_of(kv + 1, kmax)
    do q = 6, 66, 60
      write (q, '(a,i7,a,f12.5,a,2f12.5)') ' final model: cells', nused, '  rms_c', rms0, '  rms_R, rms_L', rmsv0, rmsh0
    end do
    if (ires == 1) then
      allocate (sd(nx - 2, ny - 2, nlay, 2), cov(nx - 2, ny - 2, nlay), rd(nx - 2, ny - 2, nlay, 2), rsum(nx - 2, ny - 2, nlay, 2), &
                cross(nx - 2, ny - 2, nlay, 2), tr(nx - 2, ny - 2, 2))
      call dazim_check(dazim_column_resolution_radial(dazim_handle, nx, ny, nlay, kv, c_loc(skv), kh, c_loc(skh), w(:, :, 1:kv), &
                                                      w(:, :, kv + 1:kmax), smooth_vs, damp, couple, sd, cov, rd, rsum, cross, tr, &
                                                      c_null_ptr, nempty, nbad), 'column resolution (Vsv, Vsh)')
      call write_radial_resolution('Vsv_Vsh_resolution_2step.dat', p, depz, vsf, vsh, sd, cov, rd, cross)
      rtrace = (tr(:, :, 1) + tr(:, :, 2))/2
      do q = 6, 66, 60
        write (q, '(a)') ' resolution: posterior std and resolution matrix of the last linearised step (the regulariser acts on the update)'
      end do
      call resolution_log('VsvVsh')
    end if
    call write_mod('MOD_2step', depz, vsf)
    call write_mod('MOD_Vsh_2step', depz, vsh)
    call write_vs_model('DSurfTomo_2step.inv', p, depz, vsf)
    call write_radial_model('Vsv_Vsh_model_2step.inv', p, depz, vsf, vsh)
    call write_phase_map('period_phaseV_2step.dat', p, inner_cells(nx, ny, kmax, pv))
  end subroutine

  ! the curves of both models into pv (Rayleigh periods of Vsv, then Love periods of Vsh) and, where asked, their dc/dVs tables
  subroutine tables(kernels)
    logical, intent(in) :: kernels
    type(c_ptr) :: a, b, c
    a = c_null_ptr; b = c_null_ptr; c = c_null_ptr
    if (kernels) then
      a = c_loc(svs); b = c_loc(svp); c = c_loc(srho)
    end if
    call dazim_check(dazim_dispersion_kernels_typed(dazim_handle, nx, ny, nz, vsf, depz, minthk, int(nsv, c_int), &
                                                    int(p%seg_wavetp(1:nsv), c_int), int(p%seg_veltp(1:nsv), c_int), &
                                                    int(p%seg_kmax(1:nsv), c_int), tRc(1:kv), pv(:, 1:kv), a, b, c, nfail), &
                     'Rayleigh curves and depth kernels of Vsv')
    if (nfail > 0) write (6, *) 'WARNING:improper initial value in disper - no zero found', nfail
    if (kernels) call dazim_check(dazim_vs_kernels(dazim_handle, nx, ny, nz, kv, vsf, svs, svp, srho, skv), 'dc/dVsv table')
    call dazim_check(dazim_dispersion_kernels_typed(dazim_handle, nx, ny, nz, vsh, depz, minthk, int(nsh, c_int), &
                                                    int(p%seg_wavetp(nsv + 1:p%nseg), c_int), int(p%seg_veltp(nsv + 1:p%nseg), c_int), &
                                                    int(p%seg_kmax(nsv + 1:p%nseg), c_int), tRc(kv + 1:kmax), pv(:, kv + 1:kmax), a, b, c, &
                                                    nfail), 'Love curves and depth kernels of Vsh')
    if (nfail > 0) write (6, *) 'WARNING:improper initial value in disper - no zero found', nfail
    if (kernels) call dazim_check(dazim_vs_kernels(dazim_handle, nx, ny, nz, kh, vsh, svs, svp, srho, skh), 'dc/dVsh table')
  end subroutine

  ! residual()'s RMS over the virtual periods t0..t1
  real function rms_of(t0, t1)
    integer, intent(in) :: t0, t1
    real*8 :: n
    n = count(w(:, :, t0:t1) > 0.0)
    rms_of = 0
    if (n > 0) rms_of = real(sqrt(sum(real(r(:, :, t0:t1, 1), 8)**2, mask=w(:, :, t0:t1) > 0.0)/n))
  end function

  ! the solve's predicted RMS over the periods t0..t1, from its per-period statistics
  real function after(t0, t1)
    integer, intent(in) :: t0, t1
    real*8 :: s, n
    integer :: t2
    s = 0; n = 0
    do t2 = t0, t1
      s = s + real(stats(2, t2, 1), 8)**2*count(w(:, :, t2) > 0.0)
      n = n + count(w(:, :, t2) > 0.0)
    end do
    after = 0
    if (n > 0) after = real(sqrt(s/n))
  end function

  ! w = 1/sigma_c where the map has coverage and pvRc is not 0, r = c_map - pvRc on the inner cells; rms0 over the pairs with w > 0,
  ! cnt of those pairs, nused = cells with at least one
  subroutine residual()
    integer :: i1, j1, t1
    s0 = 0; cnt = 0
    do t1 = 1, kmax
      do j1 = 1, ny - 2
        do i1 = 1, nx - 2
          col = j1*nx + i1 + 1
          w(i1, j1, t1) = wcov(i1, j1, t1)
          if (pv(col, t1) == 0) w(i1, j1, t1) = 0
          r(i1, j1, t1, 1) = real(cmap(i1, j1, t1) - pv(col, t1))
          if (w(i1, j1, t1) > 0) then
            s0 = s0 + real(r(i1, j1, t1, 1), 8)**2
            cnt = cnt + 1
          end if
        end do
      end do
    end do
    rms0 = 0
    if (cnt > 0) rms0 = real(sqrt(s0/cnt))
    nused = count(any(w > 0.0, dim=3))
  end subroutine
end program
