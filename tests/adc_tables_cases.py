"""The launch geometries of the float-ADC feeders that tests/test_gpu_adc_tables_geometry.py runs on the GPU, each with the plan
it exists for (host/adc_tables_plan.hpp: adc_tables_plan, adc_encode_plan).  tests/test_adc_tables_plan_host.py asserts on a CPU
that the header, as the library compiles it, plans every case as written here — so no GPU case is vacuous: a change of the
planner that moves a case off its geometry fails there, on a machine without a GPU.

A tables case: nq, ma, nsq, dim, opq and
  plan      what adc_tables_plan returns (grid = x, y, z);
  unhalved  the probes per workgroup before the loop that halves them until the residuals fit the LDS budget;
  last      the probes of the last probe group (na of the workgroups blockIdx.y == pgroups - 1).
An encoder case: nsq, dim, n and plan = what adc_encode_plan returns; trips = the chunks of vper vectors workgroup 0 and
workgroup 1 take, and the vectors of the last chunk of workgroup 1."""


def _plan(probes, pgroups, msplit, mper, cper, cslices, DS, grid, lds_bytes):
    return dict(probes=probes, pgroups=pgroups, msplit=msplit, mper=mper, cper=cper, cslices=cslices, DS=DS, grid=grid, lds_bytes=lds_bytes)


def _case(name, nq, ma, nsq, dim, opq, centroids, plan, unhalved, last, why):
    return dict(name=name, nq=nq, ma=ma, nsq=nsq, dim=dim, opq=bool(opq), centroids=centroids, plan=plan, unhalved=unhalved, last=last, why=why)


# 8-bit sub-quantizers (256 centroids): AdcIndex(nsq, 8).search_tables
TABLES8 = [
    _case("msplit1_halved_opq_ds120", 512, 16, 4, 480, 1, 256, _plan(8, 2, 1, 4, 1, 1, 0, (512, 2, 1), 30848), 16, 8,
          "one workgroup walks all 4 sub-quantizers; 16 probes halved to 8 by the OPQ staging; the any-size path at ds 120"),
    _case("msplit1_halved_pq_ds256", 512, 16, 4, 1024, 0, 256, _plan(8, 2, 1, 4, 1, 1, 0, (512, 2, 1), 32896), 16, 8,
          "halving without a rotation: the residuals alone exceed the budget"),
    _case("msplit_nsq_halved_opq", 40, 32, 16, 1024, 1, 256, _plan(8, 4, 16, 1, 1, 1, 0, (40, 4, 16), 34848), 16, 8,
          "halving with the sub-quantizers spread over grid.z (mper 1)"),
    _case("msplit1_probes9_short_last", 512, 17, 8, 128, 1, 256, _plan(9, 2, 1, 8, 1, 1, 16, (512, 2, 1), 9504), 9, 8,
          "probes 9 with a short last probe group (8) on the register path DS 16"),
    _case("max_dim_pq_probes2", 512, 16, 4, 4096, 0, 256, _plan(2, 8, 1, 4, 1, 1, 0, (512, 8, 1), 32800), 16, 2,
          "the largest dimension: three halvings, 16 -> 2 probes, ds 1024"),
    _case("max_dim_opq_probes1", 2, 3, 4, 4096, 1, 256, _plan(1, 3, 4, 1, 1, 1, 0, (2, 3, 4), 20484), 1, 1,
          "the largest dimension with a 4096 x 4096 rotation, one probe per workgroup"),
]

# 16-bit sub-quantizers (65536 centroids): AdcIndex.create16(nsq).search_tables
TABLES16 = [
    _case("2x16_msplit1_cper64", 512, 1, 2, 16, 0, 65536, _plan(1, 1, 1, 2, 64, 4, 8, (512, 1, 4), 72), 1, 1,
          "a workgroup walks both sub-quantizers (mper 2) and loops over 64 blocks of 256 centroids; 256 MiB of tables"),
    _case("2x16_msplit1_probes2", 512, 2, 2, 16, 1, 65536, _plan(2, 1, 1, 2, 64, 4, 8, (512, 1, 4), 272), 2, 2,
          "the same with two probes per workgroup; 512 MiB of tables in one pass of the default budget"),
    _case("4x16_ds32", 3, 5, 4, 128, 1, 65536, _plan(1, 5, 4, 1, 4, 64, 32, (3, 5, 256), 644), 1, 1,
          "4x16 on the register path DS 32"),
    _case("2x16_ds64", 3, 5, 2, 128, 0, 65536, _plan(1, 5, 2, 1, 2, 128, 0, (3, 5, 256), 260), 1, 1,
          "2x16 at 128 dimensions: ds 64, the any-size path"),
    _case("8x16_ds16", 3, 3, 8, 128, 0, 65536, _plan(1, 3, 8, 1, 8, 32, 16, (3, 3, 256), 68), 1, 1,
          "8x16 on the register path DS 16"),
]

TABLES = TABLES8 + TABLES16

# the 8-bit encoder's outer loop takes a second trip: pyqadc.adc_encode
ENCODE_ROWS = 997            # distinct vectors, tiled to n
ENCODE = [
    dict(name="vper32_second_trip", nsq=4, dim=8, n=8192 * 32 + 33, plan=dict(vper=32, DS=0, grid=8192, lds_bytes=32 * (48 + 32 + 16 + 4)),
         trips=(2, 2), last=1),
    dict(name="vper4_second_trip_dim2048", nsq=4, dim=2048, n=8192 * 4 + 5, plan=dict(vper=4, DS=0, grid=8192, lds_bytes=4 * (48 + 8192 + 16 + 4)),
         trips=(2, 2), last=1),
]


def by_name(cases, name):
    (c,) = [c for c in cases if c["name"] == name]
    return c


def table_bytes(c):
    return c["nq"] * c["ma"] * c["nsq"] * c["centroids"] * 4
