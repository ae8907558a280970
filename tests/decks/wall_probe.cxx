// wall_probe.cxx -- an input deck written for tests/test_gpu_wall_deck.py and tools/gen_wall_golden.py (deck API only): two
// species in an 8 x 4 x 4 box, periodic in y and z, whose x faces carry the two absorbing handlers the reference ships --
// absorb_tally on -x, link_boundary on +x.  q/m is zero, so the fields never act and the trajectories are those of the
// bit-exact push whatever the fields do; positions and momenta are loaded with uniform_rand only.  The reference executable
// and the HIP host therefore absorb the same particles in the same steps.  begin_diagnostics prints nabs and n_out every
// step, read as a deck reads them, and dumps both species before the first step and after the last.
// -DWALL_PROBE_RESTART_AT=k: restart files are written at step k.
// -DWALL_PROBE_HIP_HOST (the HIP host only): the host's count of particle-mirror downloads is printed too.

begin_globals {
  int tally_code, link_code;
};

begin_initialization {
  const int nx = 8, ny = 4, nz = 4, np = 3000;
  const double lx = 8, ly = 4, lz = 4;

  num_step        = 12;
  status_interval = 0;
  grid->cvac = 1;
  grid->eps0 = 1;
  grid->damp = 0;
  grid->dt   = 0.95*courant_length( lx, ly, lz, nx, ny, nz );
  define_periodic_grid( 0, 0, 0, lx, ly, lz, nx, ny, nz, 1, 1, 1 );

  species_t * light = define_species( "light", 0, 2*np, np, 0, 1 );
  species_t * heavy = define_species( "heavy", 0, 2*np, np, 0, 1 );

  absorb_tally_t at;
  memset( &at, 0, sizeof(at) );
  at.nspec = 2;
  at.id[0] = heavy->id;                 // (not in the species' order: nabs[] follows id[])
  at.id[1] = light->id;
  link_boundary_t lb;
  memset( &lb, 0, sizeof(lb) );
  strcpy( lb.fbase, "link" );
  lb.n_out = 5;                         // (the header of the file is n_out as the first write finds it)
  global->tally_code = add_boundary( grid, absorb_tally, &at );
  global->link_code  = add_boundary( grid, link_boundary, &lb );
  set_domain_field_bc( BOUNDARY(-1,0,0), pec_fields );
  set_domain_field_bc( BOUNDARY( 1,0,0), pec_fields );
  set_domain_particle_bc( BOUNDARY(-1,0,0), global->tally_code );
  set_domain_particle_bc( BOUNDARY( 1,0,0), global->link_code );
  define_material( "vacuum", 1 );
  finalize_field_advance( standard_field_advance );

  seed_rand( 20261020 );
  for( int n=0; n<np; n++ ) {
    const double x = uniform_rand( 0, lx ), y = uniform_rand( 0, ly ), z = uniform_rand( 0, lz );
    const double ux = uniform_rand( -0.7, 0.7 ), uy = uniform_rand( -0.3, 0.3 ), uz = uniform_rand( -0.3, 0.3 );
    inject_particle( light, x, y, z, ux, uy, uz, -0.002, n+1, 0, 0 );
    inject_particle( heavy, lx-x, y, z, 0.5*ux, uz, uy, 0.0075, n+1, 0, 0 );
  }
}

begin_diagnostics {
  const absorb_tally_t  * at = (const absorb_tally_t  *)grid->boundary[ -global->tally_code - 3 ].params;
  const link_boundary_t * lb = (const link_boundary_t *)grid->boundary[ -global->link_code  - 3 ].params;
  printf( "wall_probe: step %d nabs %d %d n_out %.0f np %d %d\n", (int)step, at->nabs[0], at->nabs[1], lb->n_out,
          (int)find_species( "light" )->np, (int)find_species( "heavy" )->np );
#ifdef WALL_PROBE_HIP_HOST
  printf( "wall_probe: step %d mirror downloads %lld\n", (int)step, (long long)particle_mirror_downloads() );
  { int64_t c[2]; double q[2], e[2];
    for( int f=0; f<2; f++ ) wall_tally( 3*f, find_species( "light" ), &c[f], &q[f], &e[f] );
    printf( "wall_probe: step %d light -x %lld %.9e %.9e +x %lld %.9e %.9e\n", (int)step, (long long)c[0], q[0], e[0], (long long)c[1], q[1], e[1] ); }
#endif
  fflush( stdout );
#ifdef WALL_PROBE_RESTART_AT
  if( step==WALL_PROBE_RESTART_AT ) dump_restart( "restart_wall", 0 );   // then `deck.exe restart restart_wall` goes on from here
#endif
  if( step!=0 && step!=num_step ) return;
  dump_particles( "light", "light" );
  dump_particles( "heavy", "heavy" );
}

begin_particle_collisions {}
begin_particle_injection {}
begin_current_injection {}
begin_field_injection {}
