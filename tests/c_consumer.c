/* c_consumer.c — a consumer of libcoflux that knows nothing but include/coflux.h and the C standard library: C99, no HIP
 * header, device memory through cf_device_alloc / cf_h2d / cf_d2h.  It is what a `ccall` relies on — the header alone is
 * enough to call the library — and tests/test_c_consumer.py holds every array it writes to the bits of the ctypes path.
 *
 *   c_consumer <input directory> <output file> <struct_size shortfall> <first_cell>
 *
 * The case is fixed (the test builds the same one): an 8 x 4 surface with halos 2 x 2 and ring 1, a 6 x 4 source with two
 * levels at time fraction 0.37, a uint8 mask.  Inputs are raw little-endian arrays in the input directory, named as below.
 * In order: cf_default_flux_params, cf_create; uploads; cf_interpolate_atmosphere_state, cf_compute_atmosphere_ocean_fluxes,
 * cf_compute_net_ocean_fluxes; cf_monitor_create (struct_size = sizeof(cf_monitor_desc) - shortfall, two entries, first_cell
 * as given), cf_monitor_collect, cf_monitor_count, cf_monitor_read; every output array and the record into the output file;
 * cf_destroy.  The output file is written only after every call succeeded.
 *
 * Exit status: 0 done; 2 a file could not be read or written; 3 the library refused a call (cf_last_error is printed);
 * 64 usage. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "coflux.h"

enum { NX = 8, NY = 4, HX = 2, HY = 2, RING = 1, NSX = 6, NSY = 4, LEVELS = 2 };
enum { SX = NX + 2 * HX, SY = NY + 2 * HY, CELLS = SX * SY, SOURCE = LEVELS * NSY * NSX };
enum { N_EXCHANGE = 8, N_FLUX = 9, N_NET = 8, N_MONITORED = 2 };
#define TIME_FRACTION 0.37
#define MONITOR_TIME 1234.5

static cf_ctx* ctx = NULL;

static void refused(const char* what, int rc, const cf_ctx* whose) {
    fprintf(stderr, "%s failed (%d): %s\n", what, rc, cf_last_error(whose));
    exit(3);
}

#define CHECK(call)                              \
    do {                                         \
        int rc_ = (call);                        \
        if (rc_ != 0) refused(#call, rc_, ctx);  \
    } while (0)
/* the handles made on a context report through the calling thread's last error */
#define CHECK_HANDLE(call)                        \
    do {                                          \
        int rc_ = (call);                         \
        if (rc_ != 0) refused(#call, rc_, NULL);  \
    } while (0)

static void read_input(const char* dir, const char* name, void* into, size_t bytes) {
    char path[4096];
    FILE* f;
    if (strlen(dir) + strlen(name) + 2 > sizeof path) exit(2);
    sprintf(path, "%s/%s", dir, name);
    f = fopen(path, "rb");
    if (!f || fread(into, 1, bytes, f) != bytes || fgetc(f) != EOF) {
        fprintf(stderr, "%s: not a file of %lu bytes\n", path, (unsigned long)bytes);
        exit(2);
    }
    fclose(f);
}

static void* upload(const void* host, size_t bytes) {
    void* d = cf_device_alloc(ctx, bytes);
    if (!d) refused("cf_device_alloc", -1, ctx);
    CHECK(cf_h2d(ctx, d, host, bytes));
    return d;
}

static void* upload_file(const char* dir, const char* name, size_t bytes) {
    void* host = malloc(bytes);
    void* d;
    if (!host) exit(2);
    read_input(dir, name, host, bytes);
    d = upload(host, bytes);
    free(host);
    return d;
}

static void download(FILE* out, const void* d, size_t bytes) {
    void* host = malloc(bytes);
    if (!host) exit(2);
    CHECK(cf_d2h(ctx, host, d, bytes));
    if (fwrite(host, 1, bytes, out) != bytes) exit(2);
    free(host);
}

int main(int argc, char** argv) {
    static const char* const source_names[CF_JRA55_NVARS] = {"tas.f32", "huss.f32", "psl.f32", "uas.f32", "vas.f32",
                                                             "rlds.f32", "rsds.f32", "prra.f32", "prsn.f32"};
    static const double zeros[CELLS];
    const char *dir, *out_path;
    int shortfall, k;
    int64_t first_cell, records = -1;
    cf_grid grid = {NX, NY, HX, HY, RING, 0};
    cf_flux_params params;
    cf_atmos_source src;
    cf_interp_weights w;
    cf_ocean_surface ocean;
    cf_exchange_fields atmos;
    cf_interface_fluxes fluxes;
    cf_net_ocean_fluxes net;
    cf_monitor_desc desc;
    cf_monitor* monitor = NULL;
    cf_monitor_value values[N_MONITORED];
    double times[1];
    double* exchange[N_EXCHANGE];
    double* flux[N_FLUX];
    double* net_out[N_NET];
    int32_t* iterations;
    void* owned[5 + 3 + CF_JRA55_NVARS];
    int n_owned = 0;
    FILE* out;

    if (argc != 5) {
        fprintf(stderr, "usage: c_consumer <input directory> <output file> <struct_size shortfall> <first_cell>\n");
        return 64;
    }
    dir = argv[1];
    out_path = argv[2];
    shortfall = atoi(argv[3]);
    first_cell = (int64_t)strtoll(argv[4], NULL, 10);

    /* 1. parameters and context */
    CHECK(cf_default_flux_params(&params));
    CHECK(cf_create(&ctx, 0, &grid, &params));

    /* 2. uploads */
    memset(&src, 0, sizeof src);
    for (k = 0; k < CF_JRA55_NVARS; ++k)
        src.data[k] = (const float*)(owned[n_owned++] = upload_file(dir, source_names[k], SOURCE * sizeof(float)));
    src.ns_x = NSX;
    src.ns_y = NSY;
    src.n_levels = LEVELS;
    src.level1 = 0;
    src.level2 = 1;
    src.time_fraction = TIME_FRACTION;
    memset(&w, 0, sizeof w);
    w.separable = 1;
    w.fi = (const double*)(owned[n_owned++] = upload_file(dir, "fi.f64", SX * sizeof(double)));
    w.fj = (const double*)(owned[n_owned++] = upload_file(dir, "fj.f64", SY * sizeof(double)));
    w.latitude = (const double*)(owned[n_owned++] = upload_file(dir, "latitude.f64", SY * sizeof(double)));
    ocean.T = (const double*)(owned[n_owned++] = upload_file(dir, "T.f64", CELLS * sizeof(double)));
    ocean.S = (const double*)(owned[n_owned++] = upload_file(dir, "S.f64", CELLS * sizeof(double)));
    ocean.u = (const double*)(owned[n_owned++] = upload_file(dir, "u.f64", CELLS * sizeof(double)));
    ocean.v = (const double*)(owned[n_owned++] = upload_file(dir, "v.f64", CELLS * sizeof(double)));
    ocean.mask = owned[n_owned++] = upload_file(dir, "mask.u8", CELLS);
    for (k = 0; k < N_EXCHANGE; ++k) exchange[k] = (double*)upload(zeros, sizeof zeros);
    for (k = 0; k < N_FLUX; ++k) flux[k] = (double*)upload(zeros, sizeof zeros);
    for (k = 0; k < N_NET; ++k) net_out[k] = (double*)upload(zeros, sizeof zeros);
    iterations = (int32_t*)upload(zeros, CELLS * sizeof(int32_t));
    atmos.u = exchange[0];
    atmos.v = exchange[1];
    atmos.T = exchange[2];
    atmos.p = exchange[3];
    atmos.q = exchange[4];
    atmos.Qs = exchange[5];
    atmos.Ql = exchange[6];
    atmos.Mp = exchange[7];
    fluxes.sensible_heat = flux[0];
    fluxes.latent_heat = flux[1];
    fluxes.water_vapor = flux[2];
    fluxes.x_momentum = flux[3];
    fluxes.y_momentum = flux[4];
    fluxes.temperature = flux[5];
    fluxes.friction_velocity = flux[6];
    fluxes.temperature_scale = flux[7];
    fluxes.humidity_scale = flux[8];
    fluxes.iterations = iterations;
    net.u = net_out[0];
    net.v = net_out[1];
    net.T = net_out[2];
    net.S = net_out[3];
    net.shortwave_surface_flux = net_out[4];
    net.upwelling_longwave = net_out[5];
    net.downwelling_longwave = net_out[6];
    net.downwelling_shortwave = net_out[7];

    /* 3. the three functions of update_state! */
    CHECK(cf_interpolate_atmosphere_state(ctx, &src, &w, &atmos));
    CHECK(cf_compute_atmosphere_ocean_fluxes(ctx, &ocean, &atmos, &fluxes));
    CHECK(cf_compute_net_ocean_fluxes(ctx, &ocean, &atmos, &fluxes, NULL, &w, &net));

    /* 4. one handle that takes a descriptor */
    memset(&desc, 0, sizeof desc);
    desc.struct_size = (int32_t)sizeof(cf_monitor_desc) - shortfall;
    desc.n_entries = N_MONITORED;
    desc.mask = ocean.mask;
    desc.first_cell = first_cell;
    desc.entries[0].a = fluxes.latent_heat;
    desc.entries[0].kind = CF_MONITOR_VALUE;
    desc.entries[1].a = net.T;
    desc.entries[1].kind = CF_MONITOR_ABS;
    CHECK(cf_monitor_create(ctx, &desc, 4, &monitor));
    CHECK_HANDLE(cf_monitor_collect(monitor, MONITOR_TIME));
    CHECK_HANDLE(cf_monitor_count(monitor, &records));
    if (records != 1) {
        fprintf(stderr, "cf_monitor_count says %ld records after one collection\n", (long)records);
        return 3;
    }
    memset(values, 0, sizeof values);
    CHECK_HANDLE(cf_monitor_read(monitor, 0, records, values, times));

    /* 5. every output array and the record */
    CHECK(cf_sync(ctx));
    out = fopen(out_path, "wb");
    if (!out) {
        fprintf(stderr, "%s: cannot be written\n", out_path);
        return 2;
    }
    for (k = 0; k < N_EXCHANGE; ++k) download(out, exchange[k], sizeof zeros);
    for (k = 0; k < N_FLUX; ++k) download(out, flux[k], sizeof zeros);
    download(out, iterations, CELLS * sizeof(int32_t));
    for (k = 0; k < N_NET; ++k) download(out, net_out[k], sizeof zeros);
    if (fwrite(values, sizeof values[0], N_MONITORED, out) != N_MONITORED || fwrite(times, sizeof times[0], 1, out) != 1 ||
        fclose(out) != 0)
        return 2;

    CHECK_HANDLE(cf_monitor_destroy(monitor));
    for (k = 0; k < N_EXCHANGE; ++k) CHECK(cf_device_free(ctx, exchange[k]));
    for (k = 0; k < N_FLUX; ++k) CHECK(cf_device_free(ctx, flux[k]));
    for (k = 0; k < N_NET; ++k) CHECK(cf_device_free(ctx, net_out[k]));
    CHECK(cf_device_free(ctx, iterations));
    for (k = 0; k < n_owned; ++k) CHECK(cf_device_free(ctx, owned[k]));
    CHECK(cf_destroy(ctx));
    return 0;
}
