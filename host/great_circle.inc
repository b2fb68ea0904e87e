! great_circle.inc -- shared by DAzimSurfTomo_amd and SurfPhaseMaps_amd (included in their contains sections)
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
