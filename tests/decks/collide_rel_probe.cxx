// collide_rel_probe.cxx -- an input deck written for tests/test_gpu_collide_rel_deck.py (deck API only): electrons and ions
// (mass 100) at the production reconnection deck's temperature, vth = 0.6 c, in a periodic 8 x 8 x 8 box.  Their q/m is
// zero, so the fields never act on them and only the collisions change a momentum.  The electrons start anisotropic,
// u_th,z = 2 u_th,x; begin_particle_collisions collides them among themselves and with the ions every step for four steps
// with the RELATIVISTIC pair (collide_params_t::relativistic = 1, vpic_hip_collide_relativistic on the device).
// begin_diagnostics dumps both species before the first step and after the last; the collision hook prints the host's
// count of particle-mirror downloads before and after its calls.

begin_globals {
  int unused;
};

begin_initialization {
  const int nx = 8, ny = 8, nz = 8, ppc = 48;
  const double lx = 8, ly = 8, lz = 8, vth = 0.6, mi = 100;

  num_step        = 4;
  status_interval = 0;
  grid->cvac = 1;
  grid->eps0 = 1;
  grid->damp = 0;
  grid->dt   = 0.95*courant_length( lx, ly, lz, nx, ny, nz );
  define_periodic_grid( 0, 0, 0, lx, ly, lz, nx, ny, nz, nproc(), 1, 1 );
  define_material( "vacuum", 1 );
  finalize_field_advance( standard_field_advance );

  species_t * electron = define_species( "electron", 0, 2*nx*ny*nz*ppc/nproc(), -1, 2, 1 );
  species_t * ion      = define_species( "ion",      0, 2*nx*ny*nz*ppc/nproc(), -1, 2, 1 );
  seed_rand( 20261020 );
  const double vthi = vth/sqrt( mi );
  for( int n=0; n<nx*ny*nz*ppc; n++ ) {
    const double x = uniform_rand( 0, lx ), y = uniform_rand( 0, ly ), z = uniform_rand( 0, lz );
    inject_particle( electron, x, y, z, maxwellian_rand( vth ), maxwellian_rand( vth ), 0.1 + maxwellian_rand( 2*vth ), -0.002, n+1, 0, 0 );
    inject_particle( ion,      x, y, z, maxwellian_rand( vthi ), maxwellian_rand( vthi ), maxwellian_rand( vthi ), 0.002, n+1, 0, 0 );
  }
}

begin_diagnostics {
  if( step!=0 && step!=num_step ) return;
  dump_particles( "electron", "electron" );
  dump_particles( "ion", "ion" );
  printf( "collide_rel_probe: step %d, electrons %d, ions %d\n", (int)step, (int)find_species( "electron" )->np, (int)find_species( "ion" )->np );
  fflush( stdout );
}

begin_particle_collisions {
  const long long d0 = (long long)particle_mirror_downloads();
  // masses and charges of the physical particles, cvar, every step, the seed -- and the eighth value, the relativistic pair
  const collide_params_t ee = { 1, 1, -1, -1, 4, 1, 21, 1 }, ei = { 1, 100, -1, 1, 2, 1, 22, 1 };
  collide( find_species( "electron" ), NULL, ee );
  collide( find_species( "electron" ), find_species( "ion" ), ei );
  const long long d1 = (long long)particle_mirror_downloads();
  printf( "collide_rel_probe: collisions of step %d, mirror downloads before %lld, after %lld\n", (int)step, d0, d1 );
  fflush( stdout );
}

begin_particle_injection {}
begin_current_injection {}
begin_field_injection {}
