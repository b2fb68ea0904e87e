! read_data.inc: reads the traveltime data file, inv/Main_Jt.f90:240-318.
! Shared by DAzimSurfTomo_amd (dazim_main.f90) and SurfPhaseMaps_amd (dazim_maps.f90): included in the
! program's body, it uses the including program's variables of the same names.
  inquire (file=datafile, exist=ex)
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
  open (87, file=datafile, status='old')
  dall = 0
  do
    read (87, '(a)', iostat=err) line
    if (err /= 0) exit
    if (line(1:1) /= '#') dall = dall + 1
  end do
  rewind (87)
  allocate (obst(dall), dist(dall))
  dall = 0; istep = 0; istep1 = 0; knum = 0; knumo = 12345
  do
    read (87, '(a)', iostat=err) line
    if (err /= 0) exit
    if (line(1:1) == '#') then
      read (line, *) str1, sta1_lat, sta1_lon, period, wavetp, veltp
      if (wavetp == 2 .and. veltp == 0) knum = period
      if (wavetp == 2 .and. veltp == 1) stop 'can not deal with Rayleigh wave group data'
      if (wavetp == 1 .and. veltp == 0) stop 'can not deal with Love wave phase data'
      if (wavetp == 1 .and. veltp == 1) stop 'can not deal with Love wave group data'
      if (knum < 1 .or. knum > kmax) stop 'period index in the data file exceeds kmaxRc'
      if (knum /= knumo) istep = 0
      istep = istep + 1
      if (istep > nsrc) stop 'more sources per period than para.in allows: increase max(sources, receivers)'
      istep1 = 0
      sta1_lat = (90.0 - sta1_lat)*pi/180.0
      sta1_lon = sta1_lon*pi/180.0
      scxf(istep, knum) = sta1_lat
      sczf(istep, knum) = sta1_lon
      periods(istep, knum) = period
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
      nrc1(istep, knum) = istep1
    end if
  end do
  close (87)
  write (*, '(a,i7)') ' Number of all measurements', dall
