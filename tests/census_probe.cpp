// census_probe -- the census's pure validator (csrc/gol_batch.h
// batch_census_args) from the command line, for
// tests/test_batch_census_capi.py: the refusals no call through the C ABI can
// reach cheaply (the 2^24-th ordinal).  Host code only; no device is touched.
//
//   census_probe boards width height  call begun next_call reach max_objects max_keys records_null n board
//
// call: 0 check, 1 begin, 2 add, 3 add_records, 4 read.  Prints the refusal,
// or "ok".
#include <cstdio>
#include <cstdlib>

#include "../akka-game-of-life_amd/csrc/gol_batch.h"

int main(int argc, char** argv) {
    if (argc != 13) {
        fprintf(stderr, "census_probe: 12 arguments\n");
        return 2;
    }
    auto num = [&](int i) { return strtoull(argv[i], nullptr, 0); };
    gol_batch_config cfg{};
    cfg.boards = (int32_t)num(1);
    cfg.width = (int32_t)num(2);
    cfg.height = (int32_t)num(3);
    cfg.topology = GOL_TORUS;
    golbatch::Geometry g{};
    if (const char* why = golbatch::batch_geometry(cfg, &g)) {
        printf("geometry: %s\n", why);
        return 1;
    }
    golbatch::CensusRequest r{};
    r.call = (golbatch::CensusRequest::Call)num(4);
    r.begun = num(5) != 0;
    r.next_call = num(6);
    r.reach = (int32_t)strtoll(argv[7], nullptr, 0);
    r.max_objects = (int32_t)strtoll(argv[8], nullptr, 0);
    r.max_keys = strtoll(argv[9], nullptr, 0);
    r.records_null = num(10) != 0;
    r.n = num(11);
    r.board = (uint32_t)num(12);
    const char* why = golbatch::batch_census_args(g, r);
    printf("%s\n", why ? why : "ok");
    return 0;
}
