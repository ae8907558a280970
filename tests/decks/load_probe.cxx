// load_probe.cxx -- an input deck written for tests/test_gpu_load_deck.py (deck API only): a periodic 8 x 8 x 16 box on one
// rank whose species are loaded on the device from per-cell tables (vpic_simulation::load_species_profile) -- no
// `repeat( n ) inject_particle( ... )` loop, no host record per particle.  The electrons are a force-free sheet: their drift
// turns with z, as in decks/trecon-part/turbulence.cxx, and their count per cell follows a z profile.  The ions carry two
// weights: a uniform background, and a sheet of lighter macro-particles appended behind it.  begin_diagnostics dumps both
// species before the first step and after the last and prints the host's mirror counters and the species' energies.

begin_globals {
  int unused;
};

begin_initialization {
  const int nx = 8, ny = 8, nz = 16;
  const double lx = 8, ly = 8, lz = 16, L = 2.0;

  num_step        = 4;
  status_interval = 0;
  grid->cvac = 1;
  grid->eps0 = 1;
  grid->damp = 0;
  grid->dt   = 0.95*courant_length( lx, ly, lz, nx, ny, nz );
  define_periodic_grid( 0, 0, -0.5*lz, lx, ly, 0.5*lz, nx, ny, nz, nproc(), 1, 1 );
  define_material( "vacuum", 1 );
  finalize_field_advance( standard_field_advance );

  species_t * electron = define_species( "electron", -1,  40000, -1, 2, 1 );
  species_t * ion      = define_species( "ion",    0.01,  40000, -1, 2, 1 );

  // the few lines that replace the loop: local tables (here profiles along z: tdim = 1 x 1 x nz) and one call per population
  std::vector<int32_t> count( nz ), sheet( nz );
  std::vector<float> udx( nz ), udy( nz ), uth( nz, 0.05f ), q_e( nz, -1.f/64 ), q_s( nz, 1.f/128 );
  for( int k=0; k<nz; k++ ) {
    const double z = grid->z0 + ( k + 0.5 )*grid->dz;
    count[k] = 2 + k%5;
    sheet[k] = ( k>=6 && k<10 ) ? 5 : 0;
    udx[k] = (float)(  0.3/cosh( z/L ) );                    // the drift turns from -y through +x to +y across the sheet
    udy[k] = (float)(  0.3*tanh( z/L ) );
  }
  vpic_hip_load_t d;
  memset( &d, 0, sizeof(d) );
  d.tdim[0] = 1; d.tdim[1] = 1; d.tdim[2] = nz;
  d.count = &count[0]; d.q = &q_e[0];
  d.ud[0] = &udx[0]; d.ud[1] = &udy[0];
  d.uth[0] = d.uth[1] = d.uth[2] = &uth[0];
  d.seed = 20261020; d.stream = 0; d.flags = VPIC_HIP_LOAD_TAGS; d.tag0 = 1;
  load_species_profile( electron, d );

  const int32_t four = 4;                                     // the ions' background: scalars (tdim = 1 x 1 x 1)
  const float q_b = 1.f/64, cold = 0.02f;
  memset( &d, 0, sizeof(d) );
  d.tdim[0] = d.tdim[1] = d.tdim[2] = 1;
  d.count = &four; d.q = &q_b; d.uth[0] = d.uth[1] = d.uth[2] = &cold;
  d.seed = 20261020; d.stream = 1; d.flags = VPIC_HIP_LOAD_TAGS; d.tag0 = 1;
  load_species_profile( ion, d );
  d.tdim[2] = nz;                                             // ... and the sheet behind it, at half the weight
  d.count = &sheet[0]; d.q = &q_s[0]; d.uth[0] = d.uth[1] = d.uth[2] = &uth[0];
  d.stream = 2; d.flags = VPIC_HIP_LOAD_TAGS | VPIC_HIP_LOAD_APPEND; d.tag0 = 1000001;
  load_species_profile( ion, d );
}

begin_diagnostics {
  if( step!=0 && step!=num_step ) return;
  species_t * electron = find_species( "electron" ), * ion = find_species( "ion" );
  printf( "load_probe: step %d, electrons %d, ions %d, mirror uploads %lld, energies %.9e %.9e\n", (int)step, (int)electron->np, (int)ion->np,
          (long long)particle_mirror_uploads(),
          energy_p( electron->p, electron->np, electron->q_m, interpolator, grid ), energy_p( ion->p, ion->np, ion->q_m, interpolator, grid ) );
  dump_particles( "electron", "electron" );
  dump_particles( "ion", "ion" );
  printf( "load_probe: step %d dumped, mirror uploads %lld\n", (int)step, (long long)particle_mirror_uploads() );
  fflush( stdout );
}

begin_particle_collisions {}
begin_particle_injection {}
begin_current_injection {}
begin_field_injection {}
