// hydro_select_probe.cxx -- an input deck written for tests/test_gpu_moments_select_deck.py (deck API only): one electron
// species in a periodic 16 x 8 x 8 box whose low corner is at (-8, 0, 0) and whose cells measure 2 x 1 x 0.5 (powers of two:
// the conversion between physical units and cells is exact), three particles in four cold (vth = 0.05), one hot (0.5), every
// particle with a tag of its own, four steps.  At the last step begin_diagnostics writes
//   T.4/hsel.4.0      hydro_dump( "electron", params, &sel ): all 14 moments, band format, of the particles with
//                     -2 <= x < 10, 1 <= z < 3 (PHYSICAL units) and KE >= 0.06 -- the hot ones inside a box
//   T.4/fields.4.0    field_dump: whole records, ghost voxels included
//   particles.4.0     dump_particles of the species
// in that order, and prints the host's count of particle-mirror downloads before and after the selected dump (dump_particles
// is what brings the particles to the host).  The test rebuilds the moments from the two plain dumps.

begin_globals {
  DumpParameters hd, fd;          // zero bytes, never constructed: the masks start empty
};

begin_initialization {
  const int nx = 16, ny = 8, nz = 8, ppc = 48;
  const double x0 = -8, y0 = 0, z0 = 0, x1 = 24, y1 = 8, z1 = 4;

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
  seed_rand( 20261019 );
  for( int n=0; n<nx*ny*nz*ppc; n++ ) {
    const double x = uniform_rand( x0, x1 ), y = uniform_rand( y0, y1 ), z = uniform_rand( z0, z1 );
    const double w = ( n%4==0 ) ? 0.5 : 0.05;
    inject_particle( electron, x, y, z, maxwellian_rand( w ), maxwellian_rand( w ), maxwellian_rand( w ), -0.002, n+1, 0, 0 );
  }

  global->hd.format = band;
  global->hd.stride_x = 1; global->hd.stride_y = 1; global->hd.stride_z = 1;
  sprintf( global->hd.baseDir, "." ); sprintf( global->hd.baseFileName, "hsel" );
  global->hd.output_variables( current_density | charge_density | momentum_density | ke_density | stress_tensor );
  global->fd.format = band_interleave;
  global->fd.stride_x = 1; global->fd.stride_y = 1; global->fd.stride_z = 1;
  sprintf( global->fd.baseDir, "." ); sprintf( global->fd.baseFileName, "fields" );
  global->fd.output_variables( electric | magnetic );
}

begin_diagnostics {
  if( step!=num_step ) return;
  species_t * sp = species_list;
  vpic_hip_select_t sel;
  memset( &sel, 0, sizeof(sel) );
  sel.n_sel = 3;
  sel.sel[0].coord = VPIC_HIP_COORD_X;   sel.sel[0].lo = -2;    sel.sel[0].hi = 10;
  sel.sel[1].coord = VPIC_HIP_COORD_Z;   sel.sel[1].lo = 1;     sel.sel[1].hi = 3;
  sel.sel[2].coord = VPIC_HIP_COORD_KE;  sel.sel[2].lo = 0.06;  sel.sel[2].hi = 1e300;

  const long long d0 = (long long)particle_mirror_downloads();
  hydro_dump( "electron", global->hd, &sel );
  const long long d1 = (long long)particle_mirror_downloads();
  field_dump( global->fd );
  dump_particles( "electron", "particles" );
  const long long d2 = (long long)particle_mirror_downloads();
  printf( "hydro_select_probe: np %d, mirror downloads before the selected dump %lld, after it %lld, after dump_particles %lld\n",
          (int)sp->np, d0, d1, d2 );
  fflush( stdout );
}

begin_particle_injection {}
begin_current_injection {}
begin_field_injection {}
begin_particle_collisions {}
