  ! column icol of a map file in the order SurfPhaseMaps_amd writes it (period, then latitude row, then longitude); every line's
  ! longitude, latitude and period must be para.in's inner grid and periods (1e-3)
  ! (included after the contains of a program: uses its nx, ny, kmax, tRc, goxd, gozd, dvxd, dvzd, line, vals(>= ncol) and q)
  subroutine read_map(fname, ncol, icol, out, announce)
    character(len=*), intent(in) :: fname
    integer, intent(in) :: ncol, icol
    real, intent(out) :: out(nx - 2, ny - 2, kmax)
    logical, intent(in) :: announce
    integer :: i1, j1, t1, ios
    logical :: there
    inquire (file=fname, exist=there)
    if (.not. there) then
      write (*, '(a,a,a)') ' ERROR: ', fname, ' is missing (SurfPhaseMaps_amd writes it)'
      error stop 'a map file is missing'
    end if
    open (12, file=fname, status='old', action='read')
    do t1 = 1, kmax
      do j1 = 1, ny - 2
        do i1 = 1, nx - 2
          read (12, '(a)', iostat=ios) line
          if (ios == 0) read (line, *, iostat=ios) vals(1:ncol)
          if (ios /= 0) then
            write (*, '(a,a,a)') ' ERROR: ', fname, ' has fewer lines than para.in''s inner grid times its periods'
            error stop 'a map file does not match para.in'
          end if
          if (abs(vals(3) - tRc(t1)) > 1e-3) then
            write (*, '(a,a,a,f10.4,a,f10.4)') ' ERROR: ', fname, ': its periods differ from para.in''s: ', vals(3), ' for', tRc(t1)
            error stop 'a map file does not match para.in'
          end if
          if (abs(vals(1) - (gozd + (j1 - 1)*dvzd)) > 1e-3 .or. abs(vals(2) - (goxd - (i1 - 1)*dvxd)) > 1e-3) then
            write (*, '(a,a,a,2f10.4)') ' ERROR: ', fname, ': its coordinates are not para.in''s inner grid at', vals(1:2)
            error stop 'a map file does not match para.in'
          end if
          out(i1, j1, t1) = vals(icol)
        end do
      end do
    end do
    read (12, '(a)', iostat=ios) line
    if (ios == 0 .and. len_trim(line) > 0) then
      write (*, '(a,a,a)') ' ERROR: ', fname, ' has more lines than para.in''s inner grid times its periods'
      error stop 'a map file does not match para.in'
    end if
    close (12)
    if (announce) then
      do q = 6, 66, 60
        write (q, '(a,a)') ' read ', fname
      end do
    end if
  end subroutine
