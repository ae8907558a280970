// fieldcoord_probe.cxx -- an input deck written for tests/test_gpu_fieldcoord_deck.py (deck API only): one thermal
// electron species in a periodic 16 x 8 x 8 box whose low corner is at (-8, 0, 0) and whose cells measure 2 x 1 x 0.5
// (powers of two: the conversion between physical units and cells is exact), in a magnetic and an electric field that
// vary in space (set_region_field), every particle with a tag of its own, four steps.  At the last step
// begin_diagnostics asks the host, from the resident state and with the interpolator that advance loaded for this step,
//   1  for the histogram of u_par x u_perp (64 x 48 bins) of the particles with -2 <= x < 10 and 1 <= z < 3 (PHYSICAL
//      units) -- vpic_simulation::distribution
//   2  for the particles with 0.9 <= pitch < 1, with the fields at them and their indices -- select_particles
// THEN computes both with a loop of its own over sp->p, which makes the particle mirror resident, from interpolator[p->i]:
// the fields at the particle in float as advance_p forms them, then in double exactly as include/vpic_hip.h writes the
// coordinates down.  It writes fieldcoord_helper.bin and fieldcoord_loop.bin (the 64 x 48 counts as uint64; then the
// count as int64, the particles, six floats per particle, the indices) and prints the host's count of particle-mirror
// downloads before the helpers, after them, and after the loop.

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
    inject_particle( electron, x, y, z, maxwellian_rand( vth ), maxwellian_rand( vth ), maxwellian_rand( vth ), -0.002, n+1, 0, 0 );
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
  vpic_hip_dist_t hist;
  memset( &hist, 0, sizeof(hist) );
  hist.n_axes = 2;
  hist.axis[0] = probe_axis( VPIC_HIP_COORD_U_PAR, -0.32, 0.01, 64 );
  hist.axis[1] = probe_axis( VPIC_HIP_COORD_U_PERP, 0, 0.0075, 48 );
  hist.n_sel = 2;
  hist.sel[0] = probe_range( VPIC_HIP_COORD_X, -2, 10 );
  hist.sel[1] = probe_range( VPIC_HIP_COORD_Z, 1, 3 );
  vpic_hip_select_t sel;
  memset( &sel, 0, sizeof(sel) );
  sel.n_sel = 1;
  sel.sel[0] = probe_range( VPIC_HIP_COORD_PITCH, 0.9, 1 );
  const size_t bins = (size_t)hist.axis[0].n*(size_t)hist.axis[1].n;

  std::vector<uint64_t> helper_counts( bins ), loop_counts( bins, 0 );
  std::vector<particle_t> helper_p( sp->np ), loop_p;
  std::vector<float> helper_f( 6*(size_t)sp->np ), loop_f;
  std::vector<int64_t> helper_i( sp->np ), loop_i;
  const long long d0 = (long long)particle_mirror_downloads();
  distribution( sp, &hist, &helper_counts[0] );
  const int64_t kept = select_particles( sp, &sel, sp->np, &helper_p[0], &helper_f[0], &helper_i[0] );
  if( kept>sp->np ) ERROR(( "select_particles kept %lld of at most %lld", (long long)kept, (long long)sp->np ));
  helper_p.resize( kept ); helper_f.resize( 6*(size_t)kept ); helper_i.resize( kept );
  const long long d1 = (long long)particle_mirror_downloads();

  // the same by hand, from the particle array and the interpolator
  const int sx = grid->nx+2, sy = grid->ny+2;
  for( int n=0; n<sp->np; n++ ) {
    const particle_t & p = sp->p[n];
    const interpolator_t & f = interpolator[p.i];
    const float dx = p.dx, dy = p.dy, dz = p.dz;
    float at[6];
    at[0] = ( f.ex + dy*f.dexdy ) + dz*( f.dexdz + dy*f.d2exdydz );
    at[1] = ( f.ey + dz*f.deydz ) + dx*( f.deydx + dz*f.d2eydzdx );
    at[2] = ( f.ez + dx*f.dezdx ) + dy*( f.dezdy + dx*f.d2ezdxdy );
    at[3] = f.cbx + dx*f.dcbxdx;
    at[4] = f.cby + dy*f.dcbydy;
    at[5] = f.cbz + dz*f.dcbzdz;
    const double bx = at[3], by = at[4], bz = at[5], ux = p.ux, uy = p.uy, uz = p.uz;
    const double b = sqrt( ( bx*bx + by*by ) + bz*bz );
    const double u_par = ( ( ux*bx + uy*by ) + uz*bz )/b;
    const double u2 = ( ux*ux + uy*uy ) + uz*uz;
    const double perp2 = u2 - u_par*u_par;
    const double u_perp = sqrt( perp2<0 ? 0.0 : perp2 );
    const double pitch = u_par/sqrt( u2 );
    const int cx = p.i%sx, cz = p.i/( sx*sy );
    const double x = (double)grid->x0 + (double)grid->dx*( (double)( cx-1 ) + ( (double)p.dx + 1.0 )*0.5 );
    const double z = (double)grid->z0 + (double)grid->dz*( (double)( cz-1 ) + ( (double)p.dz + 1.0 )*0.5 );
    if( x>=-2 && x<10 && z>=1 && z<3 ) {
      const double t0 = ( u_par - hist.axis[0].lo )/hist.axis[0].d, t1 = ( u_perp - hist.axis[1].lo )/hist.axis[1].d;
      if( t0>=0 && t0<hist.axis[0].n && t1>=0 && t1<hist.axis[1].n ) loop_counts[ (size_t)(int)t1*hist.axis[0].n + (int)t0 ]++;
    }
    if( pitch>=0.9 && pitch<1 ) {
      loop_p.push_back( p );
      loop_f.insert( loop_f.end(), at, at+6 );
      loop_i.push_back( n );
    }
  }
  const long long d2 = (long long)particle_mirror_downloads();

  const char * names[2] = { "fieldcoord_helper.bin", "fieldcoord_loop.bin" };
  for( int w=0; w<2; w++ ) {
    FILE * f = fopen( names[w], "wb" );
    if( !f ) ERROR(( "cannot write %s", names[w] ));
    const std::vector<particle_t> & rp = w==0 ? helper_p : loop_p;
    const std::vector<float> & rf = w==0 ? helper_f : loop_f;
    const std::vector<int64_t> & ri = w==0 ? helper_i : loop_i;
    fwrite( w==0 ? &helper_counts[0] : &loop_counts[0], sizeof(uint64_t), bins, f );
    const int64_t count = (int64_t)rp.size();
    fwrite( &count, sizeof(count), 1, f );
    if( count ) {
      fwrite( &rp[0], sizeof(particle_t), rp.size(), f );
      fwrite( &rf[0], sizeof(float), rf.size(), f );
      fwrite( &ri[0], sizeof(int64_t), ri.size(), f );
    }
    fclose( f );
  }
  printf( "fieldcoord_probe: np %d, kept %lld, mirror downloads before the helpers %lld, after the helpers %lld, after the loop %lld\n",
          (int)sp->np, (long long)kept, d0, d1, d2 );
  fflush( stdout );
}

begin_particle_injection {}
begin_current_injection {}
begin_field_injection {}
begin_particle_collisions {}
