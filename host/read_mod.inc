! read_mod.inc: reads the initial model MOD, inv/Main_Jt.f90:346-356.
! Shared by DAzimSurfTomo_amd (dazim_main.f90) and SurfPhaseMaps_amd (dazim_maps.f90): included in the
! program's body, it uses the including program's variables of the same names.
  open (11, file='MOD', status='old')
  vsf = 0
  read (11, *) (depz(i), i=1, nz)
  do k = 1, nz
    do j = 1, ny
      read (11, *) (vsf(i, j, k), i=1, nx)
    end do
  end do
  close (11)
