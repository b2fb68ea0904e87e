! read_para.inc: reads para.in, inv/Main_Jt.f90:158-214.
! Shared by DAzimSurfTomo_amd (dazim_main.f90) and SurfPhaseMaps_amd (dazim_maps.f90): included in the
! program's body, it uses the including program's variables of the same names.
  open (10, file=inputfile, status='old', action='read')
  read (10, '(a30)') dummy
  read (10, '(a30)') dummy
  read (10, '(a30)') dummy
  read (10, *) datafile
  read (10, *) nx, ny, nz
  read (10, *) goxd, gozd
  read (10, *) dvxd, dvzd
  read (10, *) minthk
  read (10, *) Minvel, Maxvel
  read (10, *) nsrc
  read (10, *) spfra
  read (10, *) maxiter
  read (10, *) iso_mod
  read (10, '(a30)') dummy
  read (10, *) weightVs
  read (10, *) weightGcs
  read (10, *) damp
  read (10, '(a30)') dummy
  read (10, *) kmaxRc
  if (kmaxRc > 0) then
    allocate (tRc(kmaxRc))
    read (10, *) (tRc(i), i=1, kmaxRc)
  end if
  close (10)
