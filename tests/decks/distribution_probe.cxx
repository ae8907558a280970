// distribution_probe.cxx -- an input deck written for tests/test_gpu_distribution_deck.py (deck API only): one thermal
// electron species in a periodic 16 x 8 x 8 box whose low corner is at (-8, 0, 0) and whose cells measure 2 x 1 x 0.5
// (powers of two: the conversion between physical units and cells is exact), four steps.  At the last step
// begin_diagnostics asks the host for three histograms of the species in PHYSICAL units
// (vpic_simulation::distribution, answered from the resident state):
//   1  x-ux, 64 x 64 bins over the whole box                                        (the histogram fits in LDS)
//   2  x-ux, 32 x 320 bins, x bins of half a cell                                   (the sliding window)
//   3  uy-LOG10_KE, 40 x 50 bins, of the particles with -2 <= x < 10, 1 <= z < 3 and KE >= 0.002
// THEN computes the same three with a loop of its own over sp->p in double, which makes the particle mirror resident,
// and writes both: distribution_helper.bin, distribution_loop.bin (4096 + 10240 + 2000 uint64 each); it prints the
// host's count of particle-mirror downloads before the helper, after it, and after the loop.

begin_globals {
  int unused;
};

begin_initialization {
  const int nx = 16, ny = 8, nz = 8, ppc = 48;
  const double x0 = -8, y0 = 0, z0 = 0, x1 = 24, y1 = 8, z1 = 4, vth = 0.1;

  num_step        = 4;
  status_interval = 0;
  grid->cvac = 1;
  grid->eps0 = 1;
  grid->damp = 0;
  grid->dt   = 0.95*courant_length( x1-x0, y1-y0, z1-z0, nx, ny, nz );
  define_periodic_grid( x0, y0, z0, x1, y1, z1, nx, ny, nz, nproc(), 1, 1 );
  define_material( "vacuum", 1 );
  finalize_field_advance( standard_field_advance );

  species_t * electron = define_species( "electron", -1, 2*nx*ny*nz*ppc/nproc(), -1, 2, 1 );
  seed_rand( 20261017 );
  for( int n=0; n<nx*ny*nz*ppc; n++ ) {
    const double x = uniform_rand( x0, x1 ), y = uniform_rand( y0, y1 ), z = uniform_rand( z0, z1 );
    // one in sixteen is ten times hotter
    const double w = ( n%16==0 ) ? 10*vth : vth;
    inject_particle( electron, x, y, z, maxwellian_rand( w ), maxwellian_rand( w ), maxwellian_rand( w ), -0.002, n, 0, 0 );
  }
}

static vpic_hip_dist_axis_t probe_axis( int coord, double lo, double d, int n ) {
  vpic_hip_dist_axis_t a; a.coord = coord; a.n = n; a.lo = lo; a.d = d; return a;
}
static vpic_hip_dist_range_t probe_range( int coord, double lo, double hi ) {
  vpic_hip_dist_range_t r; r.coord = coord; r.pad = 0; r.lo = lo; r.hi = hi; return r;
}

begin_diagnostics {
  if( step!=num_step ) return;
  species_t * sp = species_list;
  const int n_desc = 3;
  vpic_hip_dist_t desc[n_desc];
  memset( desc, 0, sizeof(desc) );
  desc[0].n_axes = 2; desc[0].axis[0] = probe_axis( VPIC_HIP_COORD_X, -8, 0.5, 64 ); desc[0].axis[1] = probe_axis( VPIC_HIP_COORD_UX, -0.4, 0.0125, 64 );
  desc[1].n_axes = 2; desc[1].axis[0] = probe_axis( VPIC_HIP_COORD_X, -8, 1.0, 32 ); desc[1].axis[1] = probe_axis( VPIC_HIP_COORD_UX, -0.4, 0.0025, 320 );
  desc[2].n_axes = 2; desc[2].axis[0] = probe_axis( VPIC_HIP_COORD_UY, -0.3, 0.015, 40 ); desc[2].axis[1] = probe_axis( VPIC_HIP_COORD_LOG10_KE, -3, 0.06, 50 );
  desc[2].n_sel = 3;
  desc[2].sel[0] = probe_range( VPIC_HIP_COORD_X, -2, 10 );
  desc[2].sel[1] = probe_range( VPIC_HIP_COORD_Z, 1, 3 );
  desc[2].sel[2] = probe_range( VPIC_HIP_COORD_KE, 0.002, 1e300 );
  size_t first[n_desc+1];
  first[0] = 0;
  for( int k=0; k<n_desc; k++ ) first[k+1] = first[k] + (size_t)desc[k].axis[0].n*(size_t)desc[k].axis[1].n;

  std::vector<uint64_t> helper( first[n_desc] ), loop( first[n_desc], 0 );
  const long long d0 = (long long)particle_mirror_downloads();
  for( int k=0; k<n_desc; k++ ) distribution( sp, &desc[k], &helper[ first[k] ] );
  const long long d1 = (long long)particle_mirror_downloads();

  // the same by hand, from the particle array, in physical units
  const int sx = grid->nx+2, sy = grid->ny+2;
  for( int n=0; n<sp->np; n++ ) {
    const particle_t & p = sp->p[n];
    const int cx = p.i%sx, cy = ( p.i/sx )%sy, cz = p.i/( sx*sy );
    double c[8];
    c[VPIC_HIP_COORD_X] = (double)grid->x0 + (double)grid->dx*( (double)( cx-1 ) + ( (double)p.dx + 1.0 )*0.5 );
    c[VPIC_HIP_COORD_Y] = (double)grid->y0 + (double)grid->dy*( (double)( cy-1 ) + ( (double)p.dy + 1.0 )*0.5 );
    c[VPIC_HIP_COORD_Z] = (double)grid->z0 + (double)grid->dz*( (double)( cz-1 ) + ( (double)p.dz + 1.0 )*0.5 );
    const double ux = p.ux, uy = p.uy, uz = p.uz;
    c[VPIC_HIP_COORD_UX] = ux; c[VPIC_HIP_COORD_UY] = uy; c[VPIC_HIP_COORD_UZ] = uz;
    c[VPIC_HIP_COORD_KE] = sqrt( ( ( 1.0 + ux*ux ) + uy*uy ) + uz*uz ) - 1.0;
    c[VPIC_HIP_COORD_LOG10_KE] = log10( c[VPIC_HIP_COORD_KE] );
    for( int k=0; k<n_desc; k++ ) {
      const vpic_hip_dist_t & d = desc[k];
      bool keep = true;
      for( int s=0; s<d.n_sel; s++ ) keep = keep && c[ d.sel[s].coord ]>=d.sel[s].lo && c[ d.sel[s].coord ]<d.sel[s].hi;
      const double t0 = ( c[ d.axis[0].coord ] - d.axis[0].lo )/d.axis[0].d, t1 = ( c[ d.axis[1].coord ] - d.axis[1].lo )/d.axis[1].d;
      if( keep && t0>=0 && t0<d.axis[0].n && t1>=0 && t1<d.axis[1].n ) loop[ first[k] + (size_t)(int)t1*d.axis[0].n + (int)t0 ]++;
    }
  }
  const long long d2 = (long long)particle_mirror_downloads();

  const char * names[2] = { "distribution_helper.bin", "distribution_loop.bin" };
  for( int w=0; w<2; w++ ) {
    FILE * f = fopen( names[w], "wb" );
    if( !f ) ERROR(( "cannot write %s", names[w] ));
    fwrite( w==0 ? &helper[0] : &loop[0], sizeof(uint64_t), first[n_desc], f );
    fclose( f );
  }
  printf( "distribution_probe: np %d, mirror downloads before the helper %lld, after the helper %lld, after the loop %lld\n",
          (int)sp->np, d0, d1, d2 );
  fflush( stdout );
}

begin_particle_injection {}
begin_current_injection {}
begin_field_injection {}
begin_particle_collisions {}
