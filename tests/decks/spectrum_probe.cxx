// spectrum_probe.cxx -- an input deck written for tests/test_gpu_spectrum_deck.py (deck API only): one thermal
// electron species in a periodic 16 x 8 x 8 box, four steps.  At the last step begin_diagnostics asks the host for the
// energy spectra of the species (vpic_simulation::energy_spectrum, answered from the resident state), THEN computes
// the same thing with a loop of its own over sp->p, which makes the particle mirror resident, and writes both:
//   spectrum_helper.bin, spectrum_loop.bin : nex * nv floats (bands per voxel, normalised, ghosts filled), nbin floats
// and prints the host's count of particle-mirror downloads before the helper, after it, and after the loop.

begin_globals {
  int unused;
};

begin_initialization {
  const int nx = 16, ny = 8, nz = 8, ppc = 48;
  const double lx = 16, ly = 8, lz = 8, vth = 0.1;

  num_step        = 4;
  status_interval = 0;
  grid->cvac = 1;
  grid->eps0 = 1;
  grid->damp = 0;
  grid->dt   = 0.95*courant_length( lx, ly, lz, nx, ny, nz );
  define_periodic_grid( 0, 0, 0, lx, ly, lz, nx, ny, nz, nproc(), 1, 1 );
  define_material( "vacuum", 1 );
  finalize_field_advance( standard_field_advance );

  species_t * electron = define_species( "electron", -1, 2*nx*ny*nz*ppc/nproc(), -1, 2, 1 );
  seed_rand( 20261016 );
  for( int n=0; n<nx*ny*nz*ppc; n++ ) {
    const double x = uniform_rand( 0, lx ), y = uniform_rand( 0, ly ), z = uniform_rand( 0, lz );
    // one in sixteen is ten times hotter: the last linear band and the upper log bins are populated too
    const double w = ( n%16==0 ) ? 10*vth : vth;
    inject_particle( electron, x, y, z, maxwellian_rand( w ), maxwellian_rand( w ), maxwellian_rand( w ), -0.002, n, 0, 0 );
  }
}

static void write_result( const char * name, const float * bands, size_t n_bands, const float * spectrum, size_t n_spectrum ) {
  FILE * f = fopen( name, "wb" );
  if( !f ) ERROR(( "cannot write %s", name ));
  fwrite( bands, sizeof(float), n_bands, f );
  fwrite( spectrum, sizeof(float), n_spectrum, f );
  fclose( f );
}

begin_diagnostics {
  if( step!=num_step ) return;
  species_t * sp = species_list;
  const int nex = 6, nbin = 800;
  const int sx = grid->nx+2, sy = grid->ny+2, sz = grid->nz+2, nv = sx*sy*sz;
  const double vth = 0.1, emax = 30;
  const double dke = emax*( vth*vth/2.0 )/nex;
  const float  e_lo = 1e-4f, e_hi = 1e4f;
  const double log_lo = log10( (double)e_lo );
  const double dloge = (double)(float)( ( log10( (double)e_hi ) - log_lo )/nbin );

  std::vector<float> bands( (size_t)nex*nv ), spectrum( nbin );
  const long long d0 = (long long)particle_mirror_downloads();
  energy_spectrum( sp, nex, dke, &bands[0], nbin, log_lo, dloge, &spectrum[0] );
  const long long d1 = (long long)particle_mirror_downloads();
  write_result( "spectrum_helper.bin", &bands[0], bands.size(), &spectrum[0], spectrum.size() );

  // the same by hand, from the particle array
  std::vector<float> b2( (size_t)nex*nv, 0.f ), s2( nbin, 0.f );
  for( int n=0; n<sp->np; n++ ) {
    const particle_t & p = sp->p[n];
    const double ux = p.ux, uy = p.uy, uz = p.uz;
    const double ke = sqrt( ( ( 1.0 + ux*ux ) + uy*uy ) + uz*uz ) - 1.0;
    int k = (int)( ke/dke );
    if( k>nex-1 ) k = nex-1;
    b2[ (size_t)k*nv + p.i ] += 1;
    const double c = ( log10( ke ) - log_lo )/dloge + 1.0;
    if( c>-1.0 && c<(double)nbin ) s2[ (int)c ] += 1;
  }
  for( int v=0; v<nv; v++ ) {
    double tot = 0;
    for( int k=0; k<nex; k++ ) tot += b2[ (size_t)k*nv + v ];
    if( tot>0 ) for( int k=0; k<nex; k++ ) b2[ (size_t)k*nv + v ] = (float)( (double)b2[ (size_t)k*nv + v ]/tot );
  }
  for( int z=0; z<sz; z++ ) for( int y=0; y<sy; y++ ) for( int x=0; x<sx; x++ ) {
    const int xi = x<1 ? 1 : x>grid->nx ? grid->nx : x, yi = y<1 ? 1 : y>grid->ny ? grid->ny : y, zi = z<1 ? 1 : z>grid->nz ? grid->nz : z;
    if( xi==x && yi==y && zi==z ) continue;
    for( int k=0; k<nex; k++ ) b2[ (size_t)k*nv + x + sx*( y + sy*z ) ] = b2[ (size_t)k*nv + xi + sx*( yi + sy*zi ) ];
  }
  const long long d2 = (long long)particle_mirror_downloads();
  write_result( "spectrum_loop.bin", &b2[0], b2.size(), &s2[0], s2.size() );
  printf( "spectrum_probe: np %d, mirror downloads before the helper %lld, after the helper %lld, after the loop %lld\n",
          (int)sp->np, d0, d1, d2 );
  fflush( stdout );
}

begin_particle_injection {}
begin_current_injection {}
begin_field_injection {}
begin_particle_collisions {}
