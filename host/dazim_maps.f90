! dazim_maps.f90 -- SurfPhaseMaps_amd: per-period Rayleigh phase-velocity maps and 2-psi anisotropy maps inverted from the data of
! the 3-D inversion program, period by period in one system, on one MI355X.
!
!   SurfPhaseMaps_amd para.in [weight_c [weight_a [uncertainty [tradeoff]]]]
!
! Inputs: the unchanged para.in, traveltime data file and MOD of DAzimSurfTomo_amd (the same readers, module dazim_io:
! read_para, read_data, read_mod).  Starting maps: MOD's dispersion curves (dazim_dispersion_kernels without kernels), the 3-D
! program's own first-iteration pvRc.  Each of para.in's iterations: eikonal fields on the current maps, map rows
! (dazim_rays_build_G_maps: dt = fdm.dc + fdmc.a1 + fdms.a2, one column block per period), CalDdatSigma weights
! (dazim_weight_data), 2-D regularisation (dazim_csr_append_laplacian2d: weight_c on the c maps, weight_a on the a1 / a2 maps;
! defaults para.in's smoothing for dVsv and for Gc,s), one LSMR over all periods with para.in's damping and the 3-D program's
! LSMR controls, and the clamped update (dazim_phase_map_update).  iso-mode T inverts c only, F c, a1 and a2 (a1, a2 solved for
! whole in every iteration, as Gc, Gs in the joint mode).
! Velocity clamp: [0.85*minvel, maxvel] of para.in -- para.in bounds shear velocities, and a Rayleigh phase velocity lies a few
! per cent below the shear velocity of the layers it samples, so the lower bound is widened by 15 %.
!
! Outputs (names distinct from the 3-D program's, so that both can run in one directory):
!   period_phaseV_map.dat    lon lat period c                           (format of period_phaseVMOD.dat)
!   period_Azm_tomo_map.inv  the nine columns of period_Azm_tomo.inv from c, a1, a2 (iso-mode F only)
!   period_map_coverage.dat  lon lat period DWS [bias]: DWS = sum |fdm| over the rays (dazim_csr_col_abs_sums); in iso-mode F
!                            the 2-psi azimuthal bias sqrt((sum fdmc)^2 + (sum fdms)^2) / DWS in [0, 1] (dazim_aprod mode 2,
!                            y = 1), 0 = even azimuthal coverage; both on the unweighted rows of the last iteration's maps
!   <para>_map.log + stdout  one line per iteration: data, mean / std / RMS of the residual before and after, LSMR istop / itn
! uncertainty = 1 (default 0: nothing below is computed or written): how well the maps are known, from dazim_map_posterior on the last
! iteration's [W G; L] (the matrix that iteration's LSMR was given) with para.in's damping: the regulariser read as a Gaussian prior,
! the data errors as CalDdatSigma's sigma.  These are the statistics of the last linearised step.
!   period_map_uncertainty.dat  lon lat period, then std_post std_noise rdiag rsum width of c; in iso-mode F also std_post rdiag of a1,
!                            std_post rdiag of a2, and leak of c (the share of c's averaging kernel that lies in a1, a2); one line
!                            per inner vertex and period in period_phaseV_map.dat's order
!   log: per period trace(Rm) / ncell per block, the median std_post of c and (iso-mode F) the median leak of c; the periods that
!                            could not be factored
! tradeoff = K >= 3 (default 0: as without the argument): which weight_c and weight_a, per period and for all periods together.  On the
! last iteration's [W G; L] and weighted right-hand side, dazim_map_tradeoff at the K factors 10^(-1 + 2k/(K-1)), k = 0 .. K-1, on
! weight_c and weight_a together with para.in's damping, and in iso-mode F a second sweep on weight_a alone (c at factor 1); both
! sweeps are the points of one call.  The maps the program inverts with do not change.
!   map_tradeoff.dat       per sweep, period and point: sweep, period, factor, the effective weights per block and the damping, m_p,
!                          chi2, |L x|^2 per block (the rows without their weight), |x|^2, tr(Rm) per block, GCV, log evidence; after a
!                          sweep's periods its totals over the periods (dazim_map_tradeoff_total), with period 0
!   log + stdout: per sweep and period, and for the totals, the L-curve corner, the GCV minimum and the evidence maximum
program SurfPhaseMaps_amd
  use iso_c_binding
  use dazim_mod
  use dazim_io
  implicit none
  character(len=100) :: inputfile, logfile
  type(para_t) :: p
  logical :: ex, iso_mod
  integer :: nx, ny, nz, nsrc, nrc, maxiter, kmax
  real :: goxd, gozd, dvxd, dvzd, minthk, Minvel, Maxvel, damp, weight_c, weight_a
  real*8, allocatable :: tRc(:)
  real, allocatable :: depz(:), vsf(:, :, :)
  real, allocatable :: scxf(:, :), sczf(:, :), rcxf(:, :, :), rczf(:, :, :)
  integer, allocatable :: periods(:, :), nrc1(:, :), nsrc1(:)
  real, allocatable :: obst(:), dist(:)
  integer :: dall, i
  ! the map inversion
  real*8, allocatable, target :: pv(:, :)
  real, allocatable :: dsyn(:), Tdata(:), datweight(:), cbst(:), dm(:), a1(:), a2(:), w(:), ustats(:, :, :), y(:), after(:)
  real, allocatable :: dws(:), sfc(:), ones(:)
  integer :: ncell, nblk, nm, iter, nar, itnlim, localSize, t1, j1, i1, q
  integer(c_int) :: nfail, istop, itn
  integer(c_int64_t) :: m64, n64, z64
  real :: minc, maxc, atol, btol, conlim, anorm, acond, rnorm, arnorm, xnorm, wstats(8), amean, astd, arms
  real :: bias
  type(c_ptr) :: G
  ! uncertainty = 1
  integer :: iunc
  integer(c_int) :: nbad
  real, allocatable, target :: upost(:, :), utrace(:, :)
  integer :: itrade                          ! tradeoff = K

  write (*, *)
  write (*, *) '                       SurfPhaseMaps'
  write (*, *)
  if (command_argument_count() < 1) stop 'usage: SurfPhaseMaps_amd para.in [weight_c [weight_a [uncertainty [tradeoff]]]]'
  call get_command_argument(1, inputfile)
  inquire (file=inputfile, exist=ex)
  if (.not. ex) stop 'unable to open the inputfile'
  call read_para(inputfile, p)
  nx = p%nx; ny = p%ny; nz = p%nz; goxd = p%goxd; gozd = p%gozd; dvxd = p%dvxd; dvzd = p%dvzd; minthk = p%minthk
  Minvel = p%Minvel; Maxvel = p%Maxvel; nsrc = p%nsrc; maxiter = p%maxiter; iso_mod = p%iso_mod; damp = p%damp; kmax = p%kmaxRc
  tRc = p%tRc
  if (nz <= 1) stop 'error nz value.'
  if (kmax <= 0) stop 'Can only deal with Rayleigh wave phase velocity data!'
  if (p%typed) call dazim_set_segments(p%nseg, p%seg_wavetp, p%seg_veltp, p%seg_kmax)
  weight_c = p%weightVs; weight_a = p%weightGcs
  call optional_arg(2, weight_c)
  call optional_arg(3, weight_a)
  iunc = 0
  call optional_arg(4, iunc)
  if (iunc /= 0 .and. iunc /= 1) then
    write (*, '(a,i0)') ' ERROR: uncertainty must be 0 or 1, not ', iunc
    error stop 'bad argument'
  end if
  if (iunc == 1 .and. maxiter < 1) error stop 'uncertainty = 1 needs at least one iteration'
  itrade = 0
  call optional_arg(5, itrade)
  if (itrade /= 0 .and. itrade < 3) then
    write (*, '(a,i6)') ' ERROR: tradeoff is 0 or the number of sweep points, at least 3; it is', itrade
    error stop 'bad tradeoff argument'
  end if
  if (itrade > 0 .and. maxiter < 1) error stop 'tradeoff > 0 needs at least one iteration'
  write (logfile, '(a,a)') trim(inputfile), '_map.log'
  open (66, file=logfile)
  write (66, *)
  write (66, *) '                  SurfPhaseMaps'
  write (66, *)
  nrc = nsrc
  minc = 0.85*Minvel; maxc = Maxvel
  ncell = (nx - 2)*(ny - 2)
  nblk = merge(1, 3, iso_mod)
  nm = ncell*kmax*nblk
  do q = 6, 66, 60
    write (q, '(a,a)') ' data file: ', trim(p%datafile)
    write (q, '(a,3i5,a,i3,a,l2)') ' grid nx ny:', nx, ny, kmax, ' periods; iterations', maxiter, '; iso-mode', iso_mod
    write (q, '(a,50f6.1)') ' periods (s):', (tRc(i), i=1, kmax)
    write (q, '(a,2f8.3,a,f8.3,a,2f8.3)') ' smoothing c, a:', weight_c, weight_a, '  damping', damp, '  c range (km/s)', minc, maxc
  end do

  call read_data(p, scxf, sczf, rcxf, rczf, periods, nrc1, nsrc1, obst, dist, dall)
  call read_mod('MOD', p, depz, vsf)

  ! ---- starting maps: MOD's dispersion curves (= the 3-D program's first-iteration pvRc) ----------------------------------------
  call dazim_init(0)
  allocate (pv(nx*ny, kmax))
  call dazim_check(dazim_dispersion_any(dazim_handle, nx, ny, nz, vsf, depz, minthk, kmax, tRc, pv, c_null_ptr, c_null_ptr, &
                                        c_null_ptr, nfail), 'starting maps')
  if (nfail > 0) write (6, *) 'WARNING:improper initial value in disper - no zero found', nfail
  allocate (dsyn(dall), Tdata(dall), datweight(dall), cbst(dall + nm), dm(nm), a1(ncell*kmax), a2(ncell*kmax), w(kmax*nblk))
  allocate (ustats(3, kmax, 3), y(dall + nm), after(dall), dws(nm), sfc(nm), ones(dall))
  a1 = 0; a2 = 0; ones = 1; dws = 0; sfc = 0
  w(1:kmax) = weight_c
  if (.not. iso_mod) w(kmax + 1:3*kmax) = weight_a
  if (iso_mod) then
    atol = 1e-3; btol = 1e-3; conlim = 1200; itnlim = 1000; localSize = nm/4
  else
    atol = 1e-5; btol = 1e-4; conlim = 200; itnlim = 500; localSize = 10
  end if
  do q = 6, 66, 60
    write (q, '(a)') '  iter   ndata   mean_in    std_in    rms_in  mean_out   std_out   rms_out  istop    itn'
  end do

  do iter = 1, maxiter
    call dazim_assemble_G_maps(.not. iso_mod, nx, ny, goxd, gozd, dvxd, dvzd, kmax, pv, periods, scxf, sczf, rcxf, rczf, nrc1, &
                               nsrc1, kmax, nsrc, nrc, dsyn, G, nar)
    ! coverage on the unweighted rows (kept from the last iteration)
    call dazim_check(dazim_csr_col_abs_sums(dazim_handle, G, dws), 'DWS')
    if (.not. iso_mod) then
      sfc = 0
      call dazim_check(dazim_aprod(dazim_handle, 2, G, sfc, ones), 'coverage sums')
    end if
    cbst = 0
    call dazim_check(dazim_weight_data(dazim_handle, G, int(dall, c_int64_t), obst, dsyn, Tdata, datweight, cbst, wstats), &
                     'data weights')
    call dazim_check(dazim_csr_append_laplacian2d(dazim_handle, G, nx, ny, kmax*nblk, w), '2-D regularisation')
    call dazim_check(dazim_csr_dims(G, m64, n64, z64), 'dims')
    dm = 0
    call dazim_check(dazim_lsmr(dazim_handle, G, cbst, damp, atol, btol, conlim, itnlim, localSize, dm, istop, itn, anorm, acond, &
                                rnorm, arnorm, xnorm), 'LSMR')
    if (iunc == 1 .and. iter == maxiter) then     ! on this iteration's [W G; L], before the update and before G is freed
      allocate (upost(nm, 6), utrace(kmax, nblk))
      upost = 0
      call dazim_check(dazim_map_posterior(dazim_handle, G, int(dall, c_int64_t), nx, ny, kmax, merge(0_c_int, 1_c_int, iso_mod), &
                                           damp, upost(:, 1), upost(:, 2), upost(:, 3), upost(:, 4), c_loc(upost(:, 5)), &
                                           merge(c_null_ptr, c_loc(upost(:, 6)), iso_mod), 0_c_int, c_null_ptr, c_null_ptr, &
                                           c_loc(utrace), nbad), 'map posterior')
    end if
    if (itrade > 0 .and. iter == maxiter) call tradeoff_sweeps()
    call dazim_check(dazim_phase_map_update(dazim_handle, nx, ny, kmax, merge(0_c_int, 1_c_int, iso_mod), pv, dm, minc, maxc, &
                                            a1, a2, ustats), 'map update')
    ! residual after: the data rows (weighted by datweight) times the applied update, unweighted again
    y = 0
    call dazim_check(dazim_aprod(dazim_handle, 1, G, dm, y), 'aprod')
    do i = 1, dall
      after(i) = Tdata(i) - y(i)/datweight(i)
    end do
    amean = sum(after)/dall
    astd = sqrt(sum((after - amean)**2)/dall)
    arms = sqrt(sum(after**2)/dall)
    do q = 6, 66, 60
      write (q, '(i6,i8,6f10.4,i7,i7)') iter, dall, wstats(1), wstats(2), wstats(4), amean, astd, arms, istop, itn
    end do
    call dazim_check(dazim_csr_free(dazim_handle, G), 'free G')
  end do

  ! ---- output files ------------------------------------------------------------------------------------------------------------
  call write_phase_map('period_phaseV_map.dat', p, inner_cells(nx, ny, kmax, pv))
  if (.not. iso_mod) then                     ! the lines of write_period_azimuthal from the maps' own a1, a2
    open (42, file='period_Azm_tomo_map.inv', status='replace', action='write')
    do t1 = 1, kmax
      do j1 = 1, ny - 2
        do i1 = 1, nx - 2
          q = (t1 - 1)*ncell + (j1 - 1)*(nx - 2) + i1
          call write_azm_line(42, gozd + (j1 - 1)*dvzd, goxd - (i1 - 1)*dvxd, tRc(t1), real(pv(j1*nx + i1 + 1, t1)), a1(q), a2(q))
        end do
      end do
    end do
    close (42)
  end if
  open (43, file='period_map_coverage.dat')
  do t1 = 1, kmax
    do j1 = 1, ny - 2
      do i1 = 1, nx - 2
        q = (t1 - 1)*ncell + (j1 - 1)*(nx - 2) + i1
        if (iso_mod) then
          write (43, '(3f10.4,es14.5)') gozd + (j1 - 1)*dvzd, goxd - (i1 - 1)*dvxd, tRc(t1), dws(q)
        else
          bias = 0.0
          if (dws(q) > 0.0) bias = min(1.0, sqrt(sfc(kmax*ncell + q)**2 + sfc(2*kmax*ncell + q)**2)/dws(q))   ! (min: rounding only)
          write (43, '(3f10.4,es14.5,f10.5)') gozd + (j1 - 1)*dvzd, goxd - (i1 - 1)*dvxd, tRc(t1), dws(q), bias
        end if
      end do
    end do
  end do
  close (43)
  if (iunc == 1) &                            ! (a period is not factored where its trace is NaN)
    call write_uncertainty('period_map_uncertainty.dat', p, 'dazim_map_posterior', 'period', tRc, 'c a1 a2', 5, upost, utrace, int(nbad), .true.)
  write (*, *) '  Program finishes successfully'
  write (66, *) '  Program finishes successfully'
  close (66)
  call dazim_finalize()

contains

  ! map_tradeoff.dat and the log's lines: dazim_map_tradeoff on this iteration's [W G; L] and weighted right-hand side cbst (the
  ! regularisation rows of G hold weight_c and weight_a, so the sweep's scale is the factor itself), before the matrix is freed.  The
  ! sweeps are the points of ONE call, sweep after sweep, so the Gram matrix of a period's data rows is formed once for both.
  subroutine tradeoff_sweeps()
    integer :: nsw, npt, s, k1, p0, p1, t2
    integer(c_int) :: corner, igcv, iev
    real, allocatable :: tscale(:, :), tdamp(:), tw(:)
    integer(c_int64_t), allocatable :: tmp(:)
    real(c_double), allocatable :: tchi2(:, :), treg2(:, :, :), txn(:, :), tlda(:, :), tldp(:, :), tdof(:, :, :), tgcv(:, :), tlev(:, :)
    real(c_double), allocatable :: tsum(:), schi2(:), ssum(:), sdof(:), sgcv(:), slev(:)
    integer(c_int), allocatable :: tbad(:, :)
    nsw = merge(1, 2, iso_mod)
    npt = nsw*itrade
    allocate (tscale(nblk, npt), tdamp(npt), tw(nblk), tmp(kmax), tchi2(kmax, npt), treg2(nblk, kmax, npt), txn(kmax, npt), tlda(kmax, npt), &
              tldp(kmax, npt), tdof(nblk, kmax, npt), tgcv(kmax, npt), tlev(kmax, npt), tbad(kmax, npt), tsum(npt), schi2(npt), ssum(npt), &
              sdof(npt), sgcv(npt), slev(npt))
    tw(1) = weight_c
    if (nblk == 3) tw(2:3) = weight_a
    tdamp = damp
    do s = 1, nsw
      do k1 = 1, itrade
        tscale(:, (s - 1)*itrade + k1) = tradeoff_factor(k1, itrade)
        if (s == 2) tscale(1, itrade + k1) = 1.0
      end do
    end do
    call dazim_check(dazim_map_tradeoff(dazim_handle, G, int(dall, c_int64_t), cbst, nx, ny, kmax, merge(0_c_int, 1_c_int, iso_mod), &
                                        int(npt, c_int), tscale, tdamp, 1_c_int, 1_c_int, tmp, tchi2, treg2, txn, tlda, tldp, tdof, tgcv, &
                                        tlev, c_null_ptr, tbad), 'map tradeoff')
    call dazim_check(dazim_map_tradeoff_total(int(npt, c_int), int(kmax, c_int), int(nblk, c_int), tmp, tchi2, treg2, tdof, tlev, schi2, &
                                              ssum, sdof, sgcv, slev), 'map tradeoff totals')
    open (45, file='map_tradeoff.dat', status='replace', action='write')
    do s = 1, nsw
      p0 = (s - 1)*itrade + 1; p1 = s*itrade
      do t2 = 1, kmax
        tsum(p0:p1) = sum(treg2(:, t2, p0:p1), dim=1)
        call dazim_check(dazim_tradeoff_pick(int(itrade, c_int), tchi2(t2, p0:p1), tsum(p0:p1), tgcv(t2, p0:p1), tlev(t2, p0:p1), corner, &
                                             igcv, iev), 'tradeoff pick')
        call write_map_tradeoff(45, 66, s, trim(merge('all blocks', 'a1 and a2 ', s == 1)), t2, tRc(t2), itrade, nblk, tw, tscale(:, p0:p1), &
                                tdamp(p0:p1), int(tmp(t2), 8), tchi2(t2, p0:p1), treg2(:, t2, p0:p1), txn(t2, p0:p1), tdof(:, t2, p0:p1), &
                                tgcv(t2, p0:p1), tlev(t2, p0:p1), int(corner), int(igcv), int(iev))
      end do
      call dazim_check(dazim_tradeoff_pick(int(itrade, c_int), schi2(p0:p1), ssum(p0:p1), sgcv(p0:p1), slev(p0:p1), corner, igcv, iev), &
                       'tradeoff pick')
      call write_map_tradeoff(45, 66, s, trim(merge('all blocks', 'a1 and a2 ', s == 1)), 0, 0d0, itrade, nblk, tw, tscale(:, p0:p1), &
                              tdamp(p0:p1), int(sum(tmp), 8), schi2(p0:p1), sum(treg2(:, :, p0:p1), dim=2), sum(txn(:, p0:p1), dim=1), &
                              sum(tdof(:, :, p0:p1), dim=2), sgcv(p0:p1), slev(p0:p1), int(corner), int(igcv), int(iev))
    end do
    close (45)
  end subroutine
end program
