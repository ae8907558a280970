// cool_probe.cxx -- an input deck written for tests/test_gpu_cool_deck.py (deck API only): a hot pair-plasma species,
// vth = 0.6 c as in the production reconnection deck, in a periodic 8 x 8 x 8 box with a uniform magnetic field cB =
// (0.5, 0.5, 0.5) from set_region_field.  Its q/m is zero, so the fields never act on it and only the cooling changes a
// momentum.  begin_particle_collisions cools it every step for four steps (vpic_simulation::cool), with one dry call
// beside it, and prints what the calls returned and the host's count of particle-mirror downloads before and after them;
// behind the last applying call two more dry calls follow one another (a dry call that wrote anything would not return
// the same twice).  begin_diagnostics dumps the species before the first step and after the last.
// Eight planted particles (tags from 1 000 001) have u = s (1, 1, 1), exactly along the loaded field.  The macro-particles
// weigh 2^-30, so the E their currents raise in four steps stays near 1e-8 and the field's direction moves by as little:
// sync |A| is then ~1e-9 of |u|, a fortieth of half a float ulp, and the planted momenta must come back bit for bit.

begin_globals {
  int unused;
};

begin_initialization {
  const int nx = 8, ny = 8, nz = 8, ppc = 48;
  const double lx = 8, ly = 8, lz = 8, vth = 0.6, w = 1.0/1073741824.0;

  num_step        = 4;
  status_interval = 0;
  grid->cvac = 1;
  grid->eps0 = 1;
  grid->damp = 0;
  grid->dt   = 0.95*courant_length( lx, ly, lz, nx, ny, nz );
  define_periodic_grid( 0, 0, 0, lx, ly, lz, nx, ny, nz, nproc(), 1, 1 );
  define_material( "vacuum", 1 );
  finalize_field_advance( standard_field_advance );
  set_region_field( everywhere, 0, 0, 0, 0.5, 0.5, 0.5 );

  species_t * electron = define_species( "electron", 0, 2*nx*ny*nz*ppc/nproc(), -1, 2, 1 );
  seed_rand( 20261021 );
  for( int n=0; n<nx*ny*nz*ppc; n++ ) {
    const double x = uniform_rand( 0, lx ), y = uniform_rand( 0, ly ), z = uniform_rand( 0, lz );
    inject_particle( electron, x, y, z, maxwellian_rand( vth ), maxwellian_rand( vth ), maxwellian_rand( vth ), -w, n+1, 0, 0 );
  }
  for( int k=0; k<8; k++ ) {
    const double s = ( k&1 ? -1 : 1 )*ldexp( 1.0, k/2 - 2 );     // +-1/4, +-1/2, +-1, +-2
    inject_particle( electron, 0.5+k, 7.5-k, 0.25+0.9*k, s, s, s, -w, 1000001+k, 0, 0 );
  }
}

begin_diagnostics {
  if( step!=0 && step!=num_step ) return;
  dump_particles( "electron", "electron" );
  printf( "cool_probe: step %d, electrons %d\n", (int)step, (int)find_species( "electron" )->np );
  fflush( stdout );
}

begin_particle_collisions {
  species_t * sp = find_species( "electron" );
  const long long d0 = (long long)particle_mirror_downloads();
  // the synchrotron rate per unit time (0.1 per step), no photon bath (it would drag the planted particles too), every
  // step, the quantum (2^-58), applying / dry
  const double quantum = ldexp( 1.0, -58 );
  const cool_params_t wet = { 0.1/grid->dt, 0, 1, quantum, 0 }, dry = { 0.1/grid->dt, 0, 1, quantum, 1 };
  const double e_dry = cool( sp, dry );
  const double e_wet = cool( sp, wet );
  const long long d1 = (long long)particle_mirror_downloads();
  printf( "cool_probe: cooling of step %d, dry %.17g, applied %.17g, mirror downloads before %lld, after %lld\n", (int)step, e_dry, e_wet, d0, d1 );
  if( step==num_step-1 ) {
    const double again1 = cool( sp, dry ), again2 = cool( sp, dry );
    printf( "cool_probe: two dry calls behind the last, %.17g and %.17g\n", again1, again2 );
  }
  fflush( stdout );
}

begin_particle_injection {}
begin_current_injection {}
begin_field_injection {}
