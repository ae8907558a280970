// select_probe.cxx -- an input deck written for tests/test_gpu_select_deck.py (deck API only): one thermal electron
// species in a periodic 16 x 8 x 8 box whose low corner is at (-8, 0, 0) and whose cells measure 2 x 1 x 0.5 (powers of
// two: the conversion between physical units and cells is exact), every particle with a tag of its own (1, 2, ...), four
// steps.  At the last step begin_diagnostics asks the host for two selections of the species, with the particles, the
// fields at them and their indices (vpic_simulation::select_particles, answered from the resident state):
//   1  the particles with -2 <= x < 10, 1 <= z < 3 (PHYSICAL units) and KE >= 0.002
//   2  every 16th tag (tag % 16 == 5)
// THEN finds the same particles with a loop of its own over sp->p, which makes the particle mirror resident, and
// interpolates the fields at them from interpolator[p->i] in float as advance_p does, and writes both:
// select_helper.bin, select_loop.bin (per selection: the count as int64, then the particles, the fields -- six floats
// per particle --, the indices); it prints the host's count of particle-mirror downloads before the helper, after it,
// and after the loop.  (The box is periodic: the array has no dead slots, so the place of a particle in sp->p after the
// download is its place on the device.)

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
  seed_rand( 20261018 );
  for( int n=0; n<nx*ny*nz*ppc; n++ ) {
    const double x = uniform_rand( x0, x1 ), y = uniform_rand( y0, y1 ), z = uniform_rand( z0, z1 );
    // one in sixteen is ten times hotter
    const double w = ( n%16==0 ) ? 10*vth : vth;
    inject_particle( electron, x, y, z, maxwellian_rand( w ), maxwellian_rand( w ), maxwellian_rand( w ), -0.002, n+1, 0, 0 );
  }
}

static vpic_hip_dist_range_t probe_range( int coord, double lo, double hi ) {
  vpic_hip_dist_range_t r; r.coord = coord; r.pad = 0; r.lo = lo; r.hi = hi; return r;
}

struct probe_records {
  std::vector<particle_t> p;
  std::vector<float> fields;
  std::vector<int64_t> index;
};

begin_diagnostics {
  if( step!=num_step ) return;
  species_t * sp = species_list;
  const int n_desc = 2;
  vpic_hip_select_t desc[n_desc];
  memset( desc, 0, sizeof(desc) );
  desc[0].n_sel = 3;
  desc[0].sel[0] = probe_range( VPIC_HIP_COORD_X, -2, 10 );
  desc[0].sel[1] = probe_range( VPIC_HIP_COORD_Z, 1, 3 );
  desc[0].sel[2] = probe_range( VPIC_HIP_COORD_KE, 0.002, 1e300 );
  desc[1].flags = VPIC_HIP_SELECT_TAG_EVERY; desc[1].tag_every = 16; desc[1].tag_phase = 5;

  probe_records helper[n_desc], loop[n_desc];
  const long long d0 = (long long)particle_mirror_downloads();
  const int64_t cap = sp->np;                                     // (a selection keeps no more than there are)
  for( int k=0; k<n_desc; k++ ) {
    helper[k].p.resize( cap ); helper[k].fields.resize( 6*(size_t)cap ); helper[k].index.resize( cap );
    const int64_t count = select_particles( sp, &desc[k], cap, &helper[k].p[0], &helper[k].fields[0], &helper[k].index[0] );
    if( count>cap ) ERROR(( "select_particles kept %lld of at most %lld", (long long)count, (long long)cap ));
    helper[k].p.resize( count ); helper[k].fields.resize( 6*(size_t)count ); helper[k].index.resize( count );
  }
  const long long d1 = (long long)particle_mirror_downloads();

  // the same by hand, from the particle array and the interpolator, in physical units
  const int sx = grid->nx+2, sy = grid->ny+2;
  for( int n=0; n<sp->np; n++ ) {
    const particle_t & p = sp->p[n];
    const int cx = p.i%sx, cz = p.i/( sx*sy );
    const double x = (double)grid->x0 + (double)grid->dx*( (double)( cx-1 ) + ( (double)p.dx + 1.0 )*0.5 );
    const double z = (double)grid->z0 + (double)grid->dz*( (double)( cz-1 ) + ( (double)p.dz + 1.0 )*0.5 );
    const double ux = p.ux, uy = p.uy, uz = p.uz;
    const double ke = sqrt( ( ( 1.0 + ux*ux ) + uy*uy ) + uz*uz ) - 1.0;
    bool keep[n_desc];
    keep[0] = x>=-2 && x<10 && z>=1 && z<3 && ke>=0.002 && ke<1e300;
    keep[1] = ( ( p.tag%16 ) + 16 )%16 == 5;
    if( !keep[0] && !keep[1] ) continue;
    const interpolator_t & f = interpolator[p.i];
    const float dx = p.dx, dy = p.dy, dz = p.dz;
    float at[6];
    at[0] = ( f.ex + dy*f.dexdy ) + dz*( f.dexdz + dy*f.d2exdydz );
    at[1] = ( f.ey + dz*f.deydz ) + dx*( f.deydx + dz*f.d2eydzdx );
    at[2] = ( f.ez + dx*f.dezdx ) + dy*( f.dezdy + dx*f.d2ezdxdy );
    at[3] = f.cbx + dx*f.dcbxdx;
    at[4] = f.cby + dy*f.dcbydy;
    at[5] = f.cbz + dz*f.dcbzdz;
    for( int k=0; k<n_desc; k++ ) if( keep[k] ) {
      loop[k].p.push_back( p );
      loop[k].fields.insert( loop[k].fields.end(), at, at+6 );
      loop[k].index.push_back( n );
    }
  }
  const long long d2 = (long long)particle_mirror_downloads();

  const char * names[2] = { "select_helper.bin", "select_loop.bin" };
  for( int w=0; w<2; w++ ) {
    FILE * f = fopen( names[w], "wb" );
    if( !f ) ERROR(( "cannot write %s", names[w] ));
    for( int k=0; k<n_desc; k++ ) {
      const probe_records & r = w==0 ? helper[k] : loop[k];
      const int64_t count = (int64_t)r.p.size();
      fwrite( &count, sizeof(count), 1, f );
      if( count ) {
        fwrite( &r.p[0], sizeof(particle_t), r.p.size(), f );
        fwrite( &r.fields[0], sizeof(float), r.fields.size(), f );
        fwrite( &r.index[0], sizeof(int64_t), r.index.size(), f );
      }
    }
    fclose( f );
  }
  printf( "select_probe: np %d, kept %lld and %lld, mirror downloads before the helper %lld, after the helper %lld, after the loop %lld\n",
          (int)sp->np, (long long)helper[0].p.size(), (long long)helper[1].p.size(), d0, d1, d2 );
  fflush( stdout );
}

begin_particle_injection {}
begin_current_injection {}
begin_field_injection {}
begin_particle_collisions {}
