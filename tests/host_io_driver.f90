! host_io_driver.f90 -- drives module dazim_io (host/dazim_io.f90) without a GPU, for tests/test_host_io_cpu.py.  Run in a
! directory that holds para.in; the first argument picks what to do:
!   roundtrip   MOD_Ref -> read_mod -> write_mod MOD_out, write_vs_model DSurfTomo_out.inv;
!               phaseV_FWD.dat -> read_map (column 4 of 4) -> write_phase_map phaseV_out.dat
!   data        read_data on para.in's data file; prints "dall <n>" and, per period, "period <k> <sources> <receivers>"
!   map FILE    read_map on FILE (column 4 of 4); prints "map ok"
!   arg [TEXT]  optional_arg on the second argument; prints "arg <value>" (0.5 without one)
program host_io_driver
  use dazim_io
  implicit none
  type(para_t) :: p
  character(len=100) :: what, fname
  real, allocatable :: depz(:), vs(:, :, :), cmap(:, :, :), scxf(:, :), sczf(:, :), rcxf(:, :, :), rczf(:, :, :), obst(:), dist(:)
  integer, allocatable :: periods(:, :), nrc1(:, :), nsrc1(:)
  integer :: dall, k
  real :: v
  call get_command_argument(1, what)
  open (66, file='driver.log')
  call read_para('para.in', p)
  allocate (cmap(p%nx - 2, p%ny - 2, p%kmaxRc))
  select case (what)
  case ('roundtrip')
    call read_mod('MOD_Ref', p, depz, vs)
    call write_mod('MOD_out', depz, vs)
    call write_vs_model('DSurfTomo_out.inv', p, depz, vs)
    call read_map('phaseV_FWD.dat', p, 4, 4, cmap, .true.)
    call write_phase_map('phaseV_out.dat', p, real(cmap, 8))
  case ('data')
    call read_data(p, scxf, sczf, rcxf, rczf, periods, nrc1, nsrc1, obst, dist, dall)
    write (*, '(a,i8)') 'dall', dall
    do k = 1, p%kmaxRc
      write (*, '(a,3i8)') 'period', k, nsrc1(k), sum(nrc1(:, k))
    end do
  case ('map')
    call get_command_argument(2, fname)
    call read_map(trim(fname), p, 4, 4, cmap, .false.)
    write (*, '(a)') 'map ok'
  case ('arg')
    v = 0.5
    call optional_arg(2, v)
    write (*, '(a,es16.8)') 'arg', v
  case default
    error stop 'host_io_driver: roundtrip | data | map FILE | arg [TEXT]'
  end select
end program
