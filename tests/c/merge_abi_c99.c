/*
 * merge_abi_c99.c -- the compaction merge's entry points as cgo sees them:
 * built with gcc -std=c99 -pedantic -Werror (tests/test_merge_abi.py).  It
 * takes the addresses of nkv_merge_records_dev and nkv_merge_records through
 * pointers of exactly the declared types, fills an nkv_run, and prints the ABI
 * version and NKV_MERGE_MAX_RUNS.  No device is touched.
 */
#include <stdint.h>
#include <stdio.h>

#include "nkv_merkle.h"

typedef int (*merge_dev_fn)(nkv_ctx *, const nkv_run *, int, void *, uint64_t, uint64_t *, uint64_t *,
                            uint64_t *, uint64_t *);
typedef int (*merge_host_fn)(nkv_ctx *, const uint8_t *const *, const uint64_t *, const uint64_t *const *,
                             const uint64_t *, int, uint8_t *, uint64_t, uint64_t *, uint64_t *, uint64_t *);

int main(void) {
    merge_dev_fn dev = nkv_merge_records_dev;
    merge_host_fn host = nkv_merge_records;
    nkv_run run;
    uint64_t n_out = 7, out_len = 7;
    run.stream = NULL;
    run.stream_len = 0;
    run.rec_off = NULL;
    run.n = 0;
    printf("abi %d\n", nkv_abi_version());
    printf("max_runs %d\n", NKV_MERGE_MAX_RUNS);
    printf("symbols %d\n", dev != NULL && host != NULL);
    /* a null context is refused before anything else happens */
    printf("null_ctx %d %d\n", dev(NULL, &run, 1, NULL, 0, NULL, NULL, &n_out, &out_len),
           host(NULL, NULL, NULL, NULL, NULL, 1, NULL, 0, NULL, &n_out, &out_len));
    return 0;
}
