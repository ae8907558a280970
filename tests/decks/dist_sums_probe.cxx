// dist_sums_probe.cxx -- an input deck written for tests/test_gpu_dist_sums_deck.py (deck API only): the box, the fields
// and the species of fieldcoord_probe.cxx -- one thermal electron species in a periodic 16 x 8 x 8 box whose low corner is
// at (-8, 0, 0) and whose cells measure 2 x 1 x 0.5 (powers of two: the conversion between physical units and cells is
// exact), in a magnetic and an electric field that vary in space -- but every particle with a weight of its own, four
// steps.  At the last step begin_diagnostics asks the host, from the resident state and with the interpolator that advance
// loaded for this step, for the ke histogram (100 bins) of the particles with -2 <= x < 10 and 1 <= z < 3 (PHYSICAL units)
// and beside it four per-bin sums: q; q ke; q E.v; (e_par v_par) X, X in LOCAL CELLS -- vpic_simulation::distribution_sums --
// the last at a quantum that refuses part of the particles.
// THEN computes all of it with a loop of its own over sp->p, which makes the particle mirror resident, from
// interpolator[p->i]: the fields at the particle in float as advance_p forms them, then in double exactly as
// include/vpic_hip.h writes the factors down, t = val / quantum, llrint(t) when fabs(t) < 2^32.  It writes
// dist_sums_helper.bin and dist_sums_loop.bin (the 100 counts as uint64, the 4 x 100 sums as int64, the four refusal counts
// as int64) and prints the host's count of particle-mirror downloads before the helper, after it, and after the loop.

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

  // a sheared guide field and a wave-like electric field: B never vanishes, and no component is the same in two cells
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
  species_t * sp = species_list;
  vpic_hip_dist_t hist;
  memset( &hist, 0, sizeof(hist) );
  hist.n_axes = 1;
  hist.axis[0] = probe_axis( VPIC_HIP_COORD_KE, 0, 0.0005, 100 );
  hist.n_sel = 2;
  hist.sel[0] = probe_range( VPIC_HIP_COORD_X, -2, 10 );
  hist.sel[1] = probe_range( VPIC_HIP_COORD_Z, 1, 3 );
  const int n_val = 4, one = VPIC_HIP_FACTOR_ONE;
  vpic_hip_dist_value_t val[n_val];
  val[0] = probe_value( VPIC_HIP_FACTOR_Q, one, one, 1e-12 );
  val[1] = probe_value( VPIC_HIP_FACTOR_Q, VPIC_HIP_COORD_KE, one, 1e-13 );
  val[2] = probe_value( VPIC_HIP_FACTOR_Q, VPIC_HIP_FACTOR_EDOTV, one, 1e-13 );
  val[3] = probe_value( VPIC_HIP_FACTOR_EPAR_VPAR, VPIC_HIP_COORD_X, one, 1e-12 );
  const size_t bins = (size_t)hist.axis[0].n;

  std::vector<uint64_t> helper_counts( bins ), loop_counts( bins, 0 );
  std::vector<int64_t> helper_sums( n_val*bins ), loop_sums( n_val*bins, 0 );
  int64_t stats[8], loop_refused[n_val] = { 0, 0, 0, 0 };
  const long long d0 = (long long)particle_mirror_downloads();
  distribution_sums( sp, &hist, val, n_val, &helper_counts[0], &helper_sums[0] );
  if( vpic_hip_species_distribution_sums_stats( resident_engine(), stats ) ) ERROR(( "no statistics" ));
  const long long d1 = (long long)particle_mirror_downloads();

  // the same by hand, from the particle array and the interpolator
  const int sx = grid->nx+2, sy = grid->ny+2;
  long long counted = 0;
  for( int n=0; n<sp->np; n++ ) {
    const particle_t & p = sp->p[n];
    const interpolator_t & f = interpolator[p.i];
    const float dx = p.dx, dy = p.dy, dz = p.dz;
    const float fex = ( f.ex + dy*f.dexdy ) + dz*( f.dexdz + dy*f.d2exdydz );
    const float fey = ( f.ey + dz*f.deydz ) + dx*( f.deydx + dz*f.d2eydzdx );
    const float fez = ( f.ez + dx*f.dezdx ) + dy*( f.dezdy + dx*f.d2ezdxdy );
    const float fbx = f.cbx + dx*f.dcbxdx, fby = f.cby + dy*f.dcbydy, fbz = f.cbz + dz*f.dcbzdz;
    const double ex = fex, ey = fey, ez = fez, bx = fbx, by = fby, bz = fbz, ux = p.ux, uy = p.uy, uz = p.uz, q = p.q;
    const double gamma = sqrt( ( ( 1.0 + ux*ux ) + uy*uy ) + uz*uz );
    const double ke = gamma - 1.0;
    const double b = sqrt( ( bx*bx + by*by ) + bz*bz );
    const double u_par = ( ( ux*bx + uy*by ) + uz*bz )/b;
    const double e_par = ( ( ex*bx + ey*by ) + ez*bz )/b;
    const double edotv = ( ( ex*ux + ey*uy ) + ez*uz )/gamma;
    const double epar_vpar = ( e_par*u_par )/gamma;
    const int cx = p.i%sx, cz = p.i/( sx*sy );
    const double x_cells = (double)( cx-1 ) + ( (double)p.dx + 1.0 )*0.5;
    const double z_cells = (double)( cz-1 ) + ( (double)p.dz + 1.0 )*0.5;
    const double x = (double)grid->x0 + (double)grid->dx*x_cells, z = (double)grid->z0 + (double)grid->dz*z_cells;
    if( !( x>=-2 && x<10 && z>=1 && z<3 ) ) continue;
    const double t0 = ( ke - hist.axis[0].lo )/hist.axis[0].d;
    if( !( t0>=0 && t0<hist.axis[0].n ) ) continue;
    const size_t bin = (size_t)(int)t0;
    loop_counts[bin]++; counted++;
    const double value[n_val] = { ( q*1.0 )*1.0, ( q*ke )*1.0, ( q*edotv )*1.0, ( epar_vpar*x_cells )*1.0 };
    for( int k=0; k<n_val; k++ ) {
      const double t = value[k]/val[k].quantum;
      if( fabs( t )<4294967296.0 ) loop_sums[ k*bins + bin ] += llrint( t );
      else loop_refused[k]++;
    }
  }
  const long long d2 = (long long)particle_mirror_downloads();

  const char * names[2] = { "dist_sums_helper.bin", "dist_sums_loop.bin" };
  for( int w=0; w<2; w++ ) {
    FILE * f = fopen( names[w], "wb" );
    if( !f ) ERROR(( "cannot write %s", names[w] ));
    fwrite( w==0 ? &helper_counts[0] : &loop_counts[0], sizeof(uint64_t), bins, f );
    fwrite( w==0 ? &helper_sums[0] : &loop_sums[0], sizeof(int64_t), n_val*bins, f );
    fwrite( w==0 ? stats+4 : loop_refused, sizeof(int64_t), n_val, f );
    fclose( f );
  }
  printf( "dist_sums_probe: np %d, counted %lld (helper %lld), mirror downloads before the helper %lld, after the helper %lld, after the loop %lld\n",
          (int)sp->np, counted, (long long)stats[2], d0, d1, d2 );
  fflush( stdout );
}

begin_particle_injection {}
begin_current_injection {}
begin_field_injection {}
begin_particle_collisions {}
