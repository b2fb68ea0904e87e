! dazim_io.f90 -- the readers and writers the host programs share: para.in, the traveltime data file, MOD and the per-period map
! files in; MOD, DSurfTomo.inv, phase-velocity maps and the two azimuthal files out; optional numeric command-line arguments.
! Every procedure gets what it needs through its arguments.  The module uses neither dazim_mod nor the HIP library, so it compiles,
! links and runs on a machine without a GPU (tests/test_host_io_cpu.py).  Output formats and the fp32 / real*8 kind of every printed
! value are those of the reference program (inv/Main_Jt.f90); compile with -O2 -ffp-contract=off like the programs.
module dazim_io
  implicit none
  private
  public :: para_t, read_para, read_data, read_mod, read_map, great_circle, inner_cells, coverage_weights, optional_arg
  public :: write_mod, write_vs_model, write_phase_map, write_azimuthal, write_period_azimuthal, write_azm_line, fast_axis
  public :: write_resolution, uncertainty_weights, tradeoff_factor, write_tradeoff, write_map_tradeoff, write_uncertainty, median
  public :: period_type, type_name, write_radial_model, write_radial_resolution

  real, parameter :: pi = 3.1415926535898
  real*8, parameter :: pi8 = real(3.1415926535898, 8)   ! the reference widens the fp32 literal too

  type para_t                                ! para.in's values under the reference's names, inv/Main_Jt.f90:158-214
    character(len=80) :: datafile
    integer :: nx, ny, nz, nsrc, maxiter, kmaxRc
    real :: goxd, gozd, dvxd, dvzd, minthk, Minvel, Maxvel, spfra, weightVs, weightGcs, damp
    logical :: iso_mod
    real*8, allocatable :: tRc(:)            ! (size 0 when kmaxRc <= 0)
    ! Wave types (DSurfTomo's dialect of para.in: after the Rayleigh phase periods up to three more optional blocks, kmaxRg, kmaxLc,
    ! kmaxLg, each positive count followed by its periods line; end of file = 0).  Everything behind the readers indexes a period
    ! number and never asks for its type, so with typed data kmaxRc and tRc hold the VIRTUAL periods: the types' periods laid end
    ! to end in the order Rc, Rg, Lc, Lg.  type_kmax / type_off: count and first virtual period - 1 of each type in that order;
    ! the segments are the types with a positive count (wavetp 2 Rayleigh / 1 Love, veltp 0 phase / 1 group, as in the data file).
    integer :: type_kmax(4) = 0, type_off(4) = 0
    integer :: nseg = 0, seg_wavetp(4) = 0, seg_veltp(4) = 0, seg_kmax(4) = 0
    logical :: typed = .false.               ! a type other than Rayleigh phase has periods
  end type
  integer, parameter :: type_wavetp(4) = [2, 2, 1, 1], type_veltp(4) = [0, 1, 0, 1]
  character(len=14), parameter :: type_names(4) = ['Rayleigh phase', 'Rayleigh group', 'Love phase    ', 'Love group    ']
  character(len=6), parameter :: type_lines(4) = ['kmaxRc', 'kmaxRg', 'kmaxLc', 'kmaxLg']

  interface optional_arg
    module procedure int_arg, int8_arg, real_arg
  end interface

contains

  subroutine read_para(inputfile, p)
    character(len=*), intent(in) :: inputfile
    type(para_t), intent(out) :: p
    character(len=40) :: dummy
    integer :: u, i, it, err, cnt(4)
    real*8 :: tt(60, 4)
    open (newunit=u, file=inputfile, status='old', action='read')
    read (u, '(a30)') dummy
    read (u, '(a30)') dummy
    read (u, '(a30)') dummy
    read (u, *) p%datafile
    read (u, *) p%nx, p%ny, p%nz
    read (u, *) p%goxd, p%gozd
    read (u, *) p%dvxd, p%dvzd
    read (u, *) p%minthk
    read (u, *) p%Minvel, p%Maxvel
    read (u, *) p%nsrc
    read (u, *) p%spfra
    read (u, *) p%maxiter
    read (u, *) p%iso_mod
    read (u, '(a30)') dummy
    read (u, *) p%weightVs
    read (u, *) p%weightGcs
    read (u, *) p%damp
    read (u, '(a30)') dummy
    read (u, *) p%kmaxRc
    allocate (p%tRc(max(p%kmaxRc, 0)))
    if (p%kmaxRc > 0) read (u, *) (p%tRc(i), i=1, p%kmaxRc)
    cnt = 0; cnt(1) = max(p%kmaxRc, 0)
    do it = 2, 4                              ! kmaxRg, kmaxLc, kmaxLg: optional, end of file = 0
      read (u, *, iostat=err) cnt(it)
      if (err /= 0) then
        cnt(it) = 0
        exit
      end if
      if (cnt(it) > 60) error stop 'para.in: more than 60 periods of one wave type'
      if (cnt(it) > 0) read (u, *) (tt(i, it), i=1, cnt(it))
      cnt(it) = max(cnt(it), 0)
    end do
    close (u)
    p%type_kmax = cnt
    do it = 1, 4
      p%type_off(it) = sum(cnt(1:it - 1))
      if (cnt(it) > 0) then
        p%nseg = p%nseg + 1
        p%seg_wavetp(p%nseg) = type_wavetp(it); p%seg_veltp(p%nseg) = type_veltp(it); p%seg_kmax(p%nseg) = cnt(it)
      end if
    end do
    p%typed = any(cnt(2:4) > 0)
    if (p%typed) then                         ! the virtual periods
      if (cnt(1) > 60) error stop 'para.in: more than 60 periods of one wave type'
      if (cnt(1) > 0) tt(1:cnt(1), 1) = p%tRc(1:cnt(1))
      deallocate (p%tRc)
      p%kmaxRc = sum(cnt)
      allocate (p%tRc(p%kmaxRc))
      do it = 1, 4
        if (cnt(it) > 0) p%tRc(p%type_off(it) + 1:p%type_off(it) + cnt(it)) = tt(1:cnt(it), it)
      end do
    end if
  end subroutine

  ! wave type of virtual period t1 in the data file's codes: wavetp 2 Rayleigh / 1 Love, veltp 0 phase / 1 group
  subroutine period_type(p, t1, wavetp, veltp)
    type(para_t), intent(in) :: p
    integer, intent(in) :: t1
    integer, intent(out) :: wavetp, veltp
    integer :: it
    wavetp = 2; veltp = 0
    do it = 1, 4
      if (t1 > p%type_off(it) .and. t1 <= p%type_off(it) + p%type_kmax(it)) then
        wavetp = type_wavetp(it); veltp = type_veltp(it)
      end if
    end do
  end subroutine

  function type_name(wavetp, veltp) result(name)
    integer, intent(in) :: wavetp, veltp
    character(len=14) :: name
    name = type_names(merge(1, 3, wavetp == 2) + merge(1, 0, veltp /= 0))
  end function

  ! the traveltime data file, inv/Main_Jt.f90:240-318: sources and receivers per period as colatitude / longitude in radians,
  ! traveltimes obst = distance / velocity.  At most nsrc receivers per source.  Unit 66 is the caller's open log.
  ! The period index of a '#' header counts within its wave type (DSurfTomo's convention); the virtual period is the type's offset
  ! plus that index, and `periods` holds virtual periods.  dper (optional): the virtual period of every datum, in file order.
  subroutine read_data(p, scxf, sczf, rcxf, rczf, periods, nrc1, nsrc1, obst, dist, dall, dper)
    type(para_t), intent(in) :: p
    real, allocatable, intent(out) :: scxf(:, :), sczf(:, :), rcxf(:, :, :), rczf(:, :, :), obst(:), dist(:)
    integer, allocatable, intent(out) :: periods(:, :), nrc1(:, :), nsrc1(:)
    integer, intent(out) :: dall
    integer, allocatable, intent(out), optional :: dper(:)
    integer :: it
    character(len=200) :: line
    character :: str1
    logical :: ex
    integer :: u, err, nsrc, nrc, kmax, istep, istep1, knum, knumo, period, wavetp, veltp
    real :: sta1_lat, sta1_lon, sta2_lat, sta2_lon, velvalue, dist1
    nsrc = p%nsrc; nrc = p%nsrc; kmax = p%kmaxRc
    inquire (file=p%datafile, exist=ex)
    if (.not. ex) then
      write (66, '(a)') 'unable to open the datafile'
      close (66)
      stop 'unable to open the datafile'
    end if
    write (*, *) 'begin load data file.....'
    allocate (scxf(nsrc, kmax), sczf(nsrc, kmax), rcxf(nrc, nsrc, kmax), rczf(nrc, nsrc, kmax))
    allocate (periods(nsrc, kmax), nrc1(nsrc, kmax), nsrc1(kmax))
    scxf = 0; sczf = 0; rcxf = 0; rczf = 0; periods = 0; nrc1 = 0; nsrc1 = 0
    ! two passes: count the data lines, then fill (the reference sizes obst by nrc*nsrc*kmax instead)
    open (newunit=u, file=p%datafile, status='old')
    dall = 0
    do
      read (u, '(a)', iostat=err) line
      if (err /= 0) exit
      if (line(1:1) /= '#') dall = dall + 1
    end do
    rewind (u)
    allocate (obst(dall), dist(dall))
    if (present(dper)) allocate (dper(dall))
    dall = 0; istep = 0; istep1 = 0; knum = 0; knumo = 12345
    do
      read (u, '(a)', iostat=err) line
      if (err /= 0) exit
      if (line(1:1) == '#') then
        read (line, *) str1, sta1_lat, sta1_lon, period, wavetp, veltp
        if ((wavetp /= 1 .and. wavetp /= 2) .or. (veltp /= 0 .and. veltp /= 1)) &
          stop 'wave type in the data file: wavetp 1 or 2, veltp 0 or 1'
        it = merge(1, 3, wavetp == 2) + veltp
        if (p%type_kmax(it) == 0 .and. it > 1) then
          write (*, '(6a)') ' ERROR: the data file holds ', trim(type_names(it)), ' data, but para.in has no ', type_lines(it), &
            ' line with a positive count and its periods (the blocks after the Rayleigh phase periods: kmaxRg, kmaxLc, kmaxLg)'
          stop 'a wave type of the data file has no periods in para.in'
        end if
        if (.not. p%typed) then
          knum = period
          if (knum < 1 .or. knum > kmax) stop 'period index in the data file exceeds kmaxRc'
        else
          if (period < 1 .or. period > p%type_kmax(it)) &
            stop 'period index in the data file exceeds the count of its wave type in para.in'
          knum = p%type_off(it) + period
        end if
        if (knum /= knumo) istep = 0
        istep = istep + 1
        if (istep > nsrc) stop 'more sources per period than para.in allows: increase max(sources, receivers)'
        istep1 = 0
        sta1_lat = (90.0 - sta1_lat)*pi/180.0
        sta1_lon = sta1_lon*pi/180.0
        scxf(istep, knum) = sta1_lat
        sczf(istep, knum) = sta1_lon
        periods(istep, knum) = knum
        nsrc1(knum) = istep
        knumo = knum
      else
        read (line, *) sta2_lat, sta2_lon, velvalue
        istep1 = istep1 + 1
        if (istep1 > nrc) stop 'more receivers per source than para.in allows: increase max(sources, receivers)'
        dall = dall + 1
        sta2_lat = (90.0 - sta2_lat)*pi/180.0
        sta2_lon = sta2_lon*pi/180.0
        rcxf(istep1, istep, knum) = sta2_lat
        rczf(istep1, istep, knum) = sta2_lon
        call great_circle(sta1_lat, sta1_lon, sta2_lat, sta2_lon, dist1)
        dist(dall) = dist1
        obst(dall) = dist1/velvalue
        if (present(dper)) dper(dall) = knum
        nrc1(istep, knum) = istep1
      end if
    end do
    close (u)
    write (*, '(a,i7)') ' Number of all measurements', dall
  end subroutine

  ! a model in the MOD format (MOD, MOD_Ref, ...), inv/Main_Jt.f90:346-356
  subroutine read_mod(fname, p, depz, vsf)
    character(len=*), intent(in) :: fname
    type(para_t), intent(in) :: p
    real, allocatable, intent(out) :: depz(:), vsf(:, :, :)
    integer :: u, i, j, k
    allocate (depz(p%nz), vsf(p%nx, p%ny, p%nz))
    open (newunit=u, file=fname, status='old')
    vsf = 0
    read (u, *) (depz(i), i=1, p%nz)
    do k = 1, p%nz
      do j = 1, p%ny
        read (u, *) (vsf(i, j, k), i=1, p%nx)
      end do
    end do
    close (u)
  end subroutine

  ! column icol of a map file in the order SurfPhaseMaps_amd writes it (period, then latitude row, then longitude); every line's
  ! longitude, latitude and period must be para.in's inner grid and periods (1e-3).  announce: ' read <file>' to stdout and unit 66.
  subroutine read_map(fname, p, ncol, icol, out, announce)
    character(len=*), intent(in) :: fname
    type(para_t), intent(in) :: p
    integer, intent(in) :: ncol, icol
    real, intent(out) :: out(p%nx - 2, p%ny - 2, p%kmaxRc)
    logical, intent(in) :: announce
    character(len=300) :: line
    real :: vals(9)
    integer :: u, i1, j1, t1, ios, q
    logical :: there
    inquire (file=fname, exist=there)
    if (.not. there) then
      write (*, '(a,a,a)') ' ERROR: ', fname, ' is missing (SurfPhaseMaps_amd writes it)'
      error stop 'a map file is missing'
    end if
    open (newunit=u, file=fname, status='old', action='read')
    do t1 = 1, p%kmaxRc
      do j1 = 1, p%ny - 2
        do i1 = 1, p%nx - 2
          read (u, '(a)', iostat=ios) line
          if (ios == 0) read (line, *, iostat=ios) vals(1:ncol)
          if (ios /= 0) then
            write (*, '(a,a,a)') ' ERROR: ', fname, ' has fewer lines than para.in''s inner grid times its periods'
            error stop 'a map file does not match para.in'
          end if
          if (abs(vals(3) - p%tRc(t1)) > 1e-3) then
            write (*, '(a,a,a,f10.4,a,f10.4)') ' ERROR: ', fname, ': its periods differ from para.in''s: ', vals(3), ' for', p%tRc(t1)
            error stop 'a map file does not match para.in'
          end if
          if (abs(vals(1) - (p%gozd + (j1 - 1)*p%dvzd)) > 1e-3 .or. abs(vals(2) - (p%goxd - (i1 - 1)*p%dvxd)) > 1e-3) then
            write (*, '(a,a,a,2f10.4)') ' ERROR: ', fname, ': its coordinates are not para.in''s inner grid at', vals(1:2)
            error stop 'a map file does not match para.in'
          end if
          out(i1, j1, t1) = vals(icol)
        end do
      end do
    end do
    read (u, '(a)', iostat=ios) line
    if (ios == 0 .and. len_trim(line) > 0) then
      write (*, '(a,a,a)') ' ERROR: ', fname, ' has more lines than para.in''s inner grid times its periods'
      error stop 'a map file does not match para.in'
    end if
    close (u)
    if (announce) then
      do q = 6, 66, 60
        write (q, '(a,a)') ' read ', fname
      end do
    end if
  end subroutine

  ! the weights of the depth and the Monte-Carlo program: 1/sigma_c on the (cell, period) pairs where period_map_coverage.dat has
  ! DWS > 0 and 0 elsewhere; 1/sigma_c everywhere without that file.  Says which to stdout and unit 66.
  subroutine coverage_weights(p, sigma_c, wcov)
    type(para_t), intent(in) :: p
    real, intent(in) :: sigma_c
    real, intent(out) :: wcov(p%nx - 2, p%ny - 2, p%kmaxRc)
    real, allocatable :: cov(:, :, :)
    logical :: have_cov
    integer :: q
    inquire (file='period_map_coverage.dat', exist=have_cov)
    if (have_cov) then
      allocate (cov(p%nx - 2, p%ny - 2, p%kmaxRc))
      call read_map('period_map_coverage.dat', p, 4, 4, cov, .true.)
      wcov = merge(1.0/sigma_c, 0.0, cov > 0.0)
      do q = 6, 66, 60
        write (q, '(a,i8,a,i8)') ' period_map_coverage.dat: weight 1/sigma_c on the (cell, period) pairs with DWS > 0:', &
          count(cov > 0.0), ' of', size(cov)
      end do
    else
      wcov = 1.0/sigma_c
      do q = 6, 66, 60
        write (q, '(a)') ' period_map_coverage.dat is absent: weight 1/sigma_c on every cell and period'
      end do
    end if
  end subroutine

  ! map_sigma = 1 of the depth program: on the pairs coverage_weights gave a weight, 1/max(sigma_c, std_post) with the posterior std
  ! of c from period_map_uncertainty.dat (its fourth column; SurfPhaseMaps_amd with uncertainty = 1), sigma_c the floor; a std that is
  ! not finite (a period that could not be factored) means no data, weight 0.  Stops when the file is missing, as read_map does.
  subroutine uncertainty_weights(p, sigma_c, wcov)
    type(para_t), intent(in) :: p
    real, intent(in) :: sigma_c
    real, intent(inout) :: wcov(p%nx - 2, p%ny - 2, p%kmaxRc)
    real, allocatable :: sd(:, :, :)
    logical, allocatable :: finite(:, :, :)
    integer :: q
    allocate (sd(p%nx - 2, p%ny - 2, p%kmaxRc), finite(p%nx - 2, p%ny - 2, p%kmaxRc))
    call read_map('period_map_uncertainty.dat', p, 4, 4, sd, .true.)
    finite = sd == sd .and. abs(sd) <= huge(sd)
    do q = 6, 66, 60
      write (q, '(a,i8,a,i8,a,i8)') ' period_map_uncertainty.dat: weight 1/max(sigma_c, std_post) on', count(wcov > 0.0 .and. finite), &
        ' (cell, period) pairs;', count(wcov > 0.0 .and. finite .and. sd <= sigma_c), ' at the floor sigma_c;', &
        count(wcov > 0.0 .and. .not. finite), ' without a finite std_post (no data)'
    end do
    where (wcov > 0.0 .and. finite)
      wcov = 1.0/max(sigma_c, sd)
    elsewhere (wcov > 0.0)
      wcov = 0.0
    end where
  end subroutine

  ! great-circle distance on a 6371 km sphere from colatitude/longitude in radians (haversine, fp32); inv/delsph.f90:1
  subroutine great_circle(colat1, lon1, colat2, lon2, del)
    real, intent(in) :: colat1, lon1, colat2, lon2
    real, intent(out) :: del
    real :: dlat, dlon, lat1, lat2, a
    dlat = colat2 - colat1
    dlon = lon2 - lon1
    lat1 = pi/2 - colat1
    lat2 = pi/2 - colat2
    a = sin(dlat/2)*sin(dlat/2) + sin(dlon/2)*sin(dlon/2)*cos(lat1)*cos(lat2)
    del = 6371.0*(2*atan2(sqrt(a), sqrt(1 - a)))
  end subroutine

  ! the inner cells of full-grid maps pv(nx*ny, kmax), in the order the map files list them
  function inner_cells(nx, ny, kmax, pv) result(c)
    integer, intent(in) :: nx, ny, kmax
    real*8, intent(in) :: pv(nx, ny, kmax)
    real*8 :: c(nx - 2, ny - 2, kmax)
    c = pv(2:nx - 1, 2:ny - 1, :)
  end function

  ! point k of npoint (1-based) of the trade-off sweep: the factor 10^(-1 + 2 (k-1)/(npoint-1)) on the regularisation weights
  real function tradeoff_factor(k, npoint)
    integer, intent(in) :: k, npoint
    tradeoff_factor = 10.0**(-1.0 + 2.0*real(k - 1)/real(npoint - 1))
  end function

  ! one sweep of dazim_model_tradeoff into tradeoff.dat (unit u, open) and the program's log (unit ulog) and stdout.  A line per
  ! point: sweep id, factor, the effective weights scale*weight per block and the damping, chi2, reg2 per block, xnorm2, dof per
  ! block, gcv, logev.  Then three lines name the points (1-based, in the file's order; `none` for -1) that dazim_tradeoff_pick chose:
  ! corner, igcv, iev are its 0-based indices.
  subroutine write_tradeoff(u, ulog, sweep, label, npoint, nblk, weights, scale, damp, chi2, reg2, xnorm2, dof, gcv, logev, corner, igcv, iev)
    integer, intent(in) :: u, ulog, sweep, npoint, nblk, corner, igcv, iev
    character(len=*), intent(in) :: label
    real, intent(in) :: weights(nblk), scale(nblk, npoint), damp(npoint)
    real*8, intent(in) :: chi2(npoint), reg2(nblk, npoint), xnorm2(npoint), dof(nblk, npoint), gcv(npoint), logev(npoint)
    integer :: k, q, which, idx(3), outs(2)
    character(len=16), parameter :: what(3) = [character(len=16) :: 'L-curve corner', 'GCV minimum', 'evidence maximum']
    do k = 1, npoint
      write (u, '(i3,30es16.7e3)') sweep, tradeoff_factor(k, npoint), scale(:, k)*weights, damp(k), chi2(k), reg2(:, k), xnorm2(k), &
        dof(:, k), gcv(k), logev(k)
    end do
    idx = [corner, igcv, iev]
    outs = [6, ulog]
    do q = 1, 2
      do which = 1, 3
        if (idx(which) < 0) then
          write (outs(q), '(a,i2,4a)') ' tradeoff sweep', sweep, ' (', label, '): ', trim(what(which))//' none'
        else
          write (outs(q), '(a,i2,4a,i4,a,es12.4)') ' tradeoff sweep', sweep, ' (', label, '): ', trim(what(which))//' at point', idx(which) + 1, &
            ', factor', tradeoff_factor(idx(which) + 1, npoint)
        end if
      end do
    end do
  end subroutine

  ! one sweep and one period of dazim_map_tradeoff into map_tradeoff.dat (unit u, open) and the program's log (unit ulog) and stdout;
  ! per = 0: the totals over the periods (dazim_map_tradeoff_total; reg2, xnorm2 and dof summed over the periods by the caller).  A
  ! line per point: sweep id, period (1-based; 0 for the totals), factor, the effective weights scale*weight per block and the
  ! damping, m_p, chi2, reg2 per block, xnorm2, dof per block, gcv, logev.  Then three lines name the points (1-based, in the file's
  ! order; `none` for -1) that dazim_tradeoff_pick chose: corner, igcv, iev are its 0-based indices.
  subroutine write_map_tradeoff(u, ulog, sweep, label, per, tper, npoint, nblk, weights, scale, damp, mp, chi2, reg2, xnorm2, dof, gcv, logev, &
                                corner, igcv, iev)
    integer, intent(in) :: u, ulog, sweep, per, npoint, nblk, corner, igcv, iev
    character(len=*), intent(in) :: label
    real*8, intent(in) :: tper
    integer(8), intent(in) :: mp
    real, intent(in) :: weights(nblk), scale(nblk, npoint), damp(npoint)
    real*8, intent(in) :: chi2(npoint), reg2(nblk, npoint), xnorm2(npoint), dof(nblk, npoint), gcv(npoint), logev(npoint)
    integer :: k, q, which, idx(3), outs(2)
    character(len=16), parameter :: what(3) = [character(len=16) :: 'L-curve corner', 'GCV minimum', 'evidence maximum']
    character(len=64) :: fmt, where
    write (fmt, '(a,i0,a)') '(i3,i5,', nblk + 2, 'es16.7e3,i10,30es16.7e3)'
    do k = 1, npoint
      write (u, fmt) sweep, per, tradeoff_factor(k, npoint), scale(:, k)*weights, damp(k), mp, chi2(k), reg2(:, k), xnorm2(k), dof(:, k), &
        gcv(k), logev(k)
    end do
    if (per == 0) then
      where = 'all periods'
    else
      write (where, '(a,i3,a,f8.2,a)') 'period', per, ' (', tper, ' s)'
    end if
    idx = [corner, igcv, iev]
    outs = [6, ulog]
    do q = 1, 2
      do which = 1, 3
        if (idx(which) < 0) then
          write (outs(q), '(a,i2,6a)') ' map tradeoff sweep', sweep, ' (', label, '), ', trim(where), ': ', trim(what(which))//' none'
        else
          write (outs(q), '(a,i2,6a,i4,a,es12.4)') ' map tradeoff sweep', sweep, ' (', label, '), ', trim(where), ': ', &
            trim(what(which))//' at point', idx(which) + 1, ', factor', tradeoff_factor(idx(which) + 1, npoint)
        end if
      end do
    end do
  end subroutine

  ! optional numeric command-line argument n: v keeps its value when there are fewer than n arguments; text that is not a
  ! number ends the program
  ! The uncertainty file of a posterior entry and the lines of stdout and the log (unit 66), for the 3-D model (axis 'depth', names
  ! 'Vs Gc Gs', ncol 6) and the maps ('period', 'c a1 a2', 5).  upost(:, 1:ncol): std_post, std_noise, rdiag, rsum and the width(s),
  ! upost(:, ncol+1) the leak, per unknown blk*size(axis)*ncell + (k-1)*ncell + (j-1)*(nx-2) + i; utrace per axis value and block.
  ! each_axis: an axis value is not factored where its trace is NaN, and the count nbad gets a line; otherwise nbad > 0 marks them all.
  subroutine write_uncertainty(fname, p, entry, axis_word, axis, names, ncol, upost, utrace, nbad, each_axis)
    character(len=*), intent(in) :: fname, entry, axis_word, names
    type(para_t), intent(in) :: p
    real*8, intent(in) :: axis(:)
    integer, intent(in) :: ncol, nbad
    real, intent(in) :: upost(:, :), utrace(:, :)
    logical, intent(in) :: each_axis
    integer :: k1, j1, i1, q, u, ncell, nb
    character(len=:), allocatable :: head, one
    ncell = (p%nx - 2)*(p%ny - 2)
    nb = size(axis)*ncell
    head = ' uncertainty '//axis_word
    one = names(1:index(names, ' ') - 1)
    open (44, file=fname, status='replace', action='write')
    do k1 = 1, size(axis)
      do j1 = 1, p%ny - 2
        do i1 = 1, p%nx - 2
          q = (k1 - 1)*ncell + (j1 - 1)*(p%nx - 2) + i1
          if (size(utrace, 2) == 1) then
            write (44, '(3f10.4,6es14.5)') p%gozd + (j1 - 1)*p%dvzd, p%goxd - (i1 - 1)*p%dvxd, axis(k1), upost(q, 1:ncol)
          else
            write (44, '(3f10.4,11es14.5)') p%gozd + (j1 - 1)*p%dvzd, p%goxd - (i1 - 1)*p%dvxd, axis(k1), upost(q, 1:ncol), &
              upost(nb + q, 1), upost(nb + q, 3), upost(2*nb + q, 1), upost(2*nb + q, 3), upost(q, ncol + 1)
          end if
        end do
      end do
    end do
    close (44)
    do u = 6, 66, 60
      write (u, '(a)') ' uncertainty: posterior std and resolution of the last linearised step ('//entry//')'
      do k1 = 1, size(axis)
        q = (k1 - 1)*ncell
        if (merge(utrace(k1, 1) /= utrace(k1, 1), nbad > 0, each_axis)) then
          write (u, '(a,f8.2,a)') head, axis(k1), ': not factored'
        else if (size(utrace, 2) == 1) then
          write (u, '(a,f8.2,a,f9.5,a,es12.4)') head, axis(k1), ': trace(Rm)/ncell '//one, utrace(k1, 1)/ncell, &
            '  median std_post '//one, median(upost(q + 1:q + ncell, 1))
        else
          write (u, '(a,f8.2,a,3f9.5,a,es12.4,a,f8.4)') head, axis(k1), ': trace(Rm)/ncell '//names, utrace(k1, :)/ncell, &
            '  median std_post '//one, median(upost(q + 1:q + ncell, 1)), '  median leak '//one, median(upost(q + 1:q + ncell, ncol + 1))
        end if
      end do
      if (each_axis .and. nbad > 0) write (u, '(a,i4)') ' uncertainty: '//axis_word//'s not factored', nbad
    end do
  end subroutine

  ! the median of v (the lower of the two middle values for an even count), by a Shell sort of a copy
  real function median(v)
    real, intent(in) :: v(:)
    real, allocatable :: s(:)
    real :: x
    integer :: m, gap, i2, j2
    s = v
    m = size(s)
    gap = m/2
    do while (gap > 0)
      do i2 = gap + 1, m
        x = s(i2); j2 = i2
        do while (j2 > gap)
          if (s(j2 - gap) <= x) exit
          s(j2) = s(j2 - gap); j2 = j2 - gap
        end do
        s(j2) = x
      end do
      gap = gap/2
    end do
    median = s((m + 1)/2)
  end function

  subroutine int_arg(n, v)
    integer, intent(in) :: n
    integer, intent(inout) :: v
    character(len=100) :: arg
    integer :: ios
    if (command_argument_count() < n) return
    call get_command_argument(n, arg)
    read (arg, *, iostat=ios) v
    if (ios /= 0) call bad_arg(n, arg)
  end subroutine

  subroutine int8_arg(n, v)
    integer, intent(in) :: n
    integer(8), intent(inout) :: v
    character(len=100) :: arg
    integer :: ios
    if (command_argument_count() < n) return
    call get_command_argument(n, arg)
    read (arg, *, iostat=ios) v
    if (ios /= 0) call bad_arg(n, arg)
  end subroutine

  subroutine real_arg(n, v)
    integer, intent(in) :: n
    real, intent(inout) :: v
    character(len=100) :: arg
    integer :: ios
    if (command_argument_count() < n) return
    call get_command_argument(n, arg)
    read (arg, *, iostat=ios) v
    if (ios /= 0) call bad_arg(n, arg)
  end subroutine

  subroutine bad_arg(n, arg)
    integer, intent(in) :: n
    character(len=*), intent(in) :: arg
    write (*, '(a,i2,a,a)') ' ERROR: argument', n, ' is not a number: ', trim(arg)
    error stop 'bad argument'
  end subroutine

  ! MOD format: the depth line, then the velocities row by row (MOD_Ref: inv/Main_Jt.f90:751-765)
  subroutine write_mod(fname, depz, vs)
    character(len=*), intent(in) :: fname
    real, intent(in) :: depz(:), vs(:, :, :)
    integer :: u, i, j, k
    open (newunit=u, file=fname)
    do k = 1, size(depz)
      write (u, '(f7.1)', advance='no') depz(k)
    end do
    do k = 1, size(vs, 3)
      do j = 1, size(vs, 2)
        do i = 1, size(vs, 1)
          if (i == 1) then
            write (u, '(/f8.4)', advance='no') vs(i, j, k)
          else
            write (u, '(f8.4)', advance='no') vs(i, j, k)
          end if
        end do
      end do
    end do
    close (u)
  end subroutine

  ! lon lat depth Vs on the whole grid, outer ring included; writeVsmodel, inv/Main_Jt.f90:838
  subroutine write_vs_model(fname, p, depz, vs)
    character(len=*), intent(in) :: fname
    type(para_t), intent(in) :: p
    real, intent(in) :: depz(:), vs(:, :, :)
    integer :: u, i, j, k
    open (newunit=u, file=fname)
    do k = 1, p%nz
      do j = 1, p%ny
        do i = 1, p%nx
          write (u, '(5f8.4)') p%gozd + (j - 2)*p%dvzd, p%goxd - (i - 2)*p%dvxd, depz(k), vs(i, j, k)
        end do
      end do
    end do
    close (u)
  end subroutine

  ! lon lat period c for the inner cells; WTPeriodPhaseV, inv/Main_Jt.f90:889
  subroutine write_phase_map(fname, p, c)
    character(len=*), intent(in) :: fname
    type(para_t), intent(in) :: p
    real*8, intent(in) :: c(p%nx - 2, p%ny - 2, p%kmaxRc)
    integer :: u, t1, j1, i1, wt, vt
    open (newunit=u, file=fname)
    do t1 = 1, p%kmaxRc
      call period_type(p, t1, wt, vt)
      do j1 = 1, p%ny - 2
        do i1 = 1, p%nx - 2
          if (p%typed) then                   ! two trailing columns: wavetp veltp
            write (u, '(4f10.4,2i3)') p%gozd + (j1 - 1)*p%dvzd, p%goxd - (i1 - 1)*p%dvxd, p%tRc(t1), c(i1, j1, t1), wt, vt
            cycle
          end if
          write (u, '(5f10.4)') p%gozd + (j1 - 1)*p%dvzd, p%goxd - (i1 - 1)*p%dvxd, p%tRc(t1), c(i1, j1, t1)
        end do
      end do
    end do
    close (u)
  end subroutine

  ! dazim_column_resolution's numbers, one line per inner cell and inverted knot in write_vs_model's order (knot, then row, then
  ! column): lon lat depth of the knot, Vs there (only with vs), std_post std_noise rdiag rsum width = res(:, :, :, 1:5)
  subroutine write_resolution(fname, p, depz, res, vs)
    character(len=*), intent(in) :: fname
    type(para_t), intent(in) :: p
    real, intent(in) :: depz(:), res(:, :, :, :)
    real, intent(in), optional :: vs(:, :, :)
    integer :: u, k1, j1, i1
    open (newunit=u, file=fname, status='replace', action='write')
    do k1 = 1, size(res, 3)
      do j1 = 1, p%ny - 2
        do i1 = 1, p%nx - 2
          write (u, '(3f10.4)', advance='no') p%gozd + (j1 - 1)*p%dvzd, p%goxd - (i1 - 1)*p%dvxd, depz(k1)
          if (present(vs)) write (u, '(f8.4)', advance='no') vs(i1 + 1, j1 + 1, k1)
          write (u, '(2f10.5,2f10.4,f10.2)') res(i1, j1, k1, 1:5)
        end do
      end do
    end do
    close (u)
  end subroutine

  ! lon lat depth Vsv Vsh Voigt-Vs xi on the whole grid in write_vs_model's order: Voigt-Vs = sqrt((2 Vsv^2 + Vsh^2) / 3),
  ! xi = (Vsh / Vsv)^2; with xi_in (inner cells, sampled knots: SurfDepthMC_amd's posterior mean of xi) that value there
  subroutine write_radial_model(fname, p, depz, vsv, vsh, xi_in)
    character(len=*), intent(in) :: fname
    type(para_t), intent(in) :: p
    real, intent(in) :: depz(:), vsv(:, :, :), vsh(:, :, :)
    real, intent(in), optional :: xi_in(:, :, :)
    integer :: u, i, j, k
    real :: xi
    open (newunit=u, file=fname, status='replace', action='write')
    do k = 1, p%nz
      do j = 1, p%ny
        do i = 1, p%nx
          xi = (vsh(i, j, k)/vsv(i, j, k))**2
          if (present(xi_in)) then
            if (i > 1 .and. i < p%nx .and. j > 1 .and. j < p%ny .and. k <= size(xi_in, 3)) xi = xi_in(i - 1, j - 1, k)
          end if
          write (u, '(6f8.4,f9.5)') p%gozd + (j - 2)*p%dvzd, p%goxd - (i - 2)*p%dvxd, depz(k), vsv(i, j, k), vsh(i, j, k), &
            sqrt((2*vsv(i, j, k)**2 + vsh(i, j, k)**2)/3), xi
        end do
      end do
    end do
    close (u)
  end subroutine

  ! dazim_column_resolution_radial's numbers, one line per inner cell and inverted knot in write_resolution's order: lon lat depth Vsv
  ! Vsh xi std_vsv std_vsh corr std_xi rdiag_v rdiag_h cross_v cross_h.  sd, rdiag, cross (:, :, knot, 1 Vsv / 2 Vsh), cov the Vsv-Vsh
  ! covariance of a knot; corr = cov / (std_vsv std_vsh) (0 where a std is 0) and, to first order in the errors,
  ! std_xi = 2 xi sqrt(max(0, (std_vsh / Vsh)^2 + (std_vsv / Vsv)^2 - 2 cov / (Vsv Vsh)))
  subroutine write_radial_resolution(fname, p, depz, vsv, vsh, sd, cov, rdiag, cross)
    character(len=*), intent(in) :: fname
    type(para_t), intent(in) :: p
    real, intent(in) :: depz(:), vsv(:, :, :), vsh(:, :, :), sd(:, :, :, :), cov(:, :, :), rdiag(:, :, :, :), cross(:, :, :, :)
    integer :: u, k1, j1, i1
    real :: v, h, xi, corr, sxi
    open (newunit=u, file=fname, status='replace', action='write')
    do k1 = 1, size(cov, 3)
      do j1 = 1, p%ny - 2
        do i1 = 1, p%nx - 2
          v = vsv(i1 + 1, j1 + 1, k1); h = vsh(i1 + 1, j1 + 1, k1)
          xi = (h/v)**2
          corr = 0
          if (sd(i1, j1, k1, 1) > 0 .and. sd(i1, j1, k1, 2) > 0) corr = cov(i1, j1, k1)/(sd(i1, j1, k1, 1)*sd(i1, j1, k1, 2))
          sxi = 2*xi*sqrt(max(0.0, (sd(i1, j1, k1, 2)/h)**2 + (sd(i1, j1, k1, 1)/v)**2 - 2*cov(i1, j1, k1)/(v*h)))
          write (u, '(3f10.4,2f8.4,f9.5,2f10.5,f9.5,f10.5,4f10.4)') p%gozd + (j1 - 1)*p%dvzd, p%goxd - (i1 - 1)*p%dvxd, depz(k1), v, h, &
            xi, sd(i1, j1, k1, 1), sd(i1, j1, k1, 2), corr, sxi, rdiag(i1, j1, k1, 1), rdiag(i1, j1, k1, 2), cross(i1, j1, k1, 1), &
            cross(i1, j1, k1, 2)
        end do
      end do
    end do
    close (u)
  end subroutine

  ! fast-axis angle in degrees, [0, 180), of the 2-psi terms (c2, s2)
  real function fast_axis(c2, s2) result(ang)
    real, intent(in) :: c2, s2
    ang = atan2(s2, c2)/pi8*180
    if (ang < 0.0) ang = ang + 360
    ang = 0.5*ang
  end function

  ! lon lat depth Vs fast-axis angle, amplitude, Gc/L %, Gs/L %; writeAzimuthal, inv/Main_Jt.f90:859
  subroutine write_azimuthal(fname, p, depz, vs, gc, gs)
    character(len=*), intent(in) :: fname
    type(para_t), intent(in) :: p
    real, intent(in) :: depz(:), vs(:, :, :), gc(:, :, :), gs(:, :, :)
    integer :: u, k1, j1, i1
    real :: c2, s2
    open (newunit=u, file=fname)
    do k1 = 1, p%nz - 1
      do j1 = 1, p%ny - 2
        do i1 = 1, p%nx - 2
          c2 = gc(i1, j1, k1); s2 = gs(i1, j1, k1)
          write (u, '(8f10.4)') p%gozd + (j1 - 1)*p%dvzd, p%goxd - (i1 - 1)*p%dvxd, depz(k1 + 1), &
            (vs(i1 + 1, j1 + 1, k1) + vs(i1 + 1, j1 + 1, k1 + 1))/2, fast_axis(c2, s2), 0.5*sqrt(c2**2 + s2**2), c2*100, s2*100
        end do
      end do
    end do
    close (u)
  end subroutine

  ! one line of a period_Azm_tomo file: lon lat period c, fast-axis angle, amplitude relative to c, amplitude, and the 2-psi terms
  ! c2, s2 themselves (isoC: c in fp32, as the reference holds it)
  ! wavetp, veltp (both or neither): two trailing columns, written with typed data only
  subroutine write_azm_line(u, lon, lat, period, isoC, c2, s2, wavetp, veltp)
    integer, intent(in) :: u
    real, intent(in) :: lon, lat, isoC, c2, s2
    real*8, intent(in) :: period
    integer, intent(in), optional :: wavetp, veltp
    real :: amp
    amp = sqrt(c2**2 + s2**2)
    if (present(wavetp) .and. present(veltp)) then
      write (u, '(9f10.5,2i3)') lon, lat, period, isoC, fast_axis(c2, s2), amp/isoC, amp, c2, s2, wavetp, veltp
      return
    end if
    write (u, '(10f10.5)') lon, lat, period, isoC, fast_axis(c2, s2), amp/isoC, amp, c2, s2
  end subroutine

  ! period maps of the 2-psi terms A1 = sum_k Lsen*Gc, A2 = sum_k Lsen*Gs; inv/FwdAzimuthalAniMap.f90:1.  lsen on the full grid,
  ! gc, gs and c on the inner cells.
  subroutine write_period_azimuthal(fname, p, lsen, gc, gs, c)
    character(len=*), intent(in) :: fname
    type(para_t), intent(in) :: p
    real, intent(in) :: lsen(p%nx*p%ny, p%kmaxRc, p%nz - 1), gc(:, :, :), gs(:, :, :)
    real*8, intent(in) :: c(p%nx - 2, p%ny - 2, p%kmaxRc)
    integer :: u, t1, j1, i1, k1, wt, vt
    real :: c2, s2
    open (newunit=u, file=fname, status='replace', action='write')
    do t1 = 1, p%kmaxRc
      call period_type(p, t1, wt, vt)
      do j1 = 1, p%ny - 2
        do i1 = 1, p%nx - 2
          c2 = 0.0; s2 = 0.0
          do k1 = 1, p%nz - 1
            c2 = c2 + lsen(j1*p%nx + i1 + 1, t1, k1)*gc(i1, j1, k1)
            s2 = s2 + lsen(j1*p%nx + i1 + 1, t1, k1)*gs(i1, j1, k1)
          end do
          if (p%typed) then
            call write_azm_line(u, p%gozd + (j1 - 1)*p%dvzd, p%goxd - (i1 - 1)*p%dvxd, p%tRc(t1), real(c(i1, j1, t1)), c2, s2, wt, vt)
          else
            call write_azm_line(u, p%gozd + (j1 - 1)*p%dvzd, p%goxd - (i1 - 1)*p%dvxd, p%tRc(t1), real(c(i1, j1, t1)), c2, s2)
          end if
        end do
      end do
    end do
    close (u)
  end subroutine
end module
