// cell_dist_probe.cxx -- an input deck written for tests/test_gpu_cell_dist_deck.py (deck API only): the box, the fields and
// the species of dist_sums_probe.cxx -- one thermal electron species, every particle with a weight of its own, in a
// periodic 16 x 8 x 8 box whose low corner is at (-8, 0, 0) and whose cells measure 2 x 1 x 0.5 (powers of two: the
// conversion between physical units and cells is exact), in a magnetic and an electric field that vary in space -- four
// steps.  At the last step begin_diagnostics writes the electrons' moments (dump_hydro: the hydro array on the device then
// holds them) and asks the host, from the field and hydro arrays on the device, for a map over x and z in PHYSICAL units --
// eight bins of two cells in x from -8, eight bins of one cell in z from 0 -- of the cells with 1 <= y < 7 (physical: the
// six inner rows) and 0.5 <= |cB| < 10 at their centre, with four sums beside the counts: J.E, at a quantum that refuses part
// of the cells; the electrons' charge density; Ex at the centre times X in LOCAL CELLS; one -- vpic_simulation::cell_distribution.  THEN it writes the field array
// (dump_fields, which brings it to the host), so that the test restates the map from the deck's own dumps.  It writes
// cell_dist_helper.bin: the 64 counts as uint64, the 4 x 64 sums as int64, the eight statistics as int64.

begin_globals {
  int unused;
};

begin_initialization {
  const int nx = 16, ny = 8, nz = 8, ppc = 48;
  const double x0 = -8, y0 = 0, z0 = 0, x1 = 24, y1 = 8, z1 = 4, vth = 0.1;
  const double kx = 2*M_PI/( x1-x0 ), ky = 2*M_PI/( y1-y0 ), kz = 2*M_PI/( z1-z0 );

  num_step        = 4;
  status_interval = 0;
  grid->cvac = 1;
  grid->eps0 = 1;
  grid->damp = 0;
  grid->dt   = 0.95*courant_length( x1-x0, y1-y0, z1-z0, nx, ny, nz );
  define_periodic_grid( x0, y0, z0, x1, y1, z1, nx, ny, nz, nproc(), 1, 1 );
  define_material( "vacuum", 1 );
  finalize_field_advance( standard_field_advance );

  // a sheared guide field and a wave-like electric field: no component is the same in two cells
  set_region_field( everywhere,
                    0.05*cos( ky*y ), 0.04*sin( kz*z ), 0.03*cos( kx*x ),
                    0.5 + 0.2*sin( ky*y ), 0.3*cos( kz*z ), 0.25*sin( kx*x ) );

  species_t * electron = define_species( "electron", -1, 2*nx*ny*nz*ppc/nproc(), -1, 2, 1 );
  seed_rand( 20261019 );
  for( int n=0; n<nx*ny*nz*ppc; n++ ) {
    const double x = uniform_rand( x0, x1 ), y = uniform_rand( y0, y1 ), z = uniform_rand( z0, z1 );
    inject_particle( electron, x, y, z, maxwellian_rand( vth ), maxwellian_rand( vth ), maxwellian_rand( vth ), -0.001*uniform_rand( 1, 3 ), n+1, 0, 0 );
  }
}

static vpic_hip_dist_axis_t probe_axis( int coord, double lo, double d, int n ) {
  vpic_hip_dist_axis_t a; a.coord = coord; a.n = n; a.lo = lo; a.d = d; return a;
}
static vpic_hip_dist_range_t probe_range( int coord, double lo, double hi ) {
  vpic_hip_dist_range_t r; r.coord = coord; r.pad = 0; r.lo = lo; r.hi = hi; return r;
}
static vpic_hip_dist_value_t probe_value( int f0, int f1, int f2, double quantum ) {
  vpic_hip_dist_value_t v; v.factor[0] = f0; v.factor[1] = f1; v.factor[2] = f2; v.pad = 0; v.quantum = quantum; return v;
}

begin_diagnostics {
  if( step!=num_step ) return;
  dump_hydro( "electron", "cell_dist_hydro" );
  vpic_hip_dist_t map;
  memset( &map, 0, sizeof(map) );
  map.n_axes = 2;
  map.axis[0] = probe_axis( VPIC_HIP_CELL_X, -8, 4, 8 );
  map.axis[1] = probe_axis( VPIC_HIP_CELL_Z, 0, 0.5, 8 );
  map.n_sel = 2;
  map.sel[0] = probe_range( VPIC_HIP_CELL_Y, 1, 7 );
  map.sel[1] = probe_range( VPIC_HIP_CELL_B_C, 0.5, 10 );
  const int n_val = 4, one = VPIC_HIP_CELL_ONE;
  vpic_hip_dist_value_t val[n_val];
  val[0] = probe_value( VPIC_HIP_CELL_JDOTE_C, one, one, 1e-12 );
  val[1] = probe_value( VPIC_HIP_CELL_H_RHO, one, one, 1e-10 );
  val[2] = probe_value( VPIC_HIP_CELL_EX_C, VPIC_HIP_CELL_X, one, 1e-9 );
  val[3] = probe_value( one, one, one, 1 );
  const size_t bins = (size_t)map.axis[0].n*(size_t)map.axis[1].n;

  std::vector<uint64_t> counts( bins );
  std::vector<int64_t> sums( n_val*bins );
  int64_t stats[8];
  cell_distribution( &map, val, n_val, &counts[0], &sums[0] );
  if( vpic_hip_cell_distribution_stats( resident_engine(), stats ) ) ERROR(( "no statistics" ));
  dump_fields( "cell_dist_fields" );

  FILE * f = fopen( "cell_dist_helper.bin", "wb" );
  if( !f ) ERROR(( "cannot write cell_dist_helper.bin" ));
  fwrite( &counts[0], sizeof(uint64_t), bins, f );
  fwrite( &sums[0], sizeof(int64_t), n_val*bins, f );
  fwrite( stats, sizeof(int64_t), 8, f );
  fclose( f );
  printf( "cell_dist_probe: cells %lld, kept %lld, counted %lld, through global memory %lld\n",
          (long long)stats[0], (long long)stats[1], (long long)stats[2], (long long)stats[3] );
  fflush( stdout );
}

begin_particle_injection {}
begin_current_injection {}
begin_field_injection {}
begin_particle_collisions {}
