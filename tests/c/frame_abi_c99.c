/*
 * frame_abi_c99.c -- the framing entry points as cgo sees them: built with gcc
 * -std=c99 -pedantic -Werror (tests/test_frame_abi.py).  It takes the addresses
 * of the two entries through pointers of exactly the declared types and prints
 * the ABI version, the constants and the status a null context gets.  No device
 * is touched.
 */
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include "nkv_merkle.h"

typedef int (*frame_dev_fn)(nkv_ctx *, const void *, uint64_t, const uint64_t *, uint64_t, int, uint64_t *, uint64_t,
                            uint64_t *, uint64_t *, uint64_t *, uint64_t *);
typedef int (*frame_fn)(nkv_ctx *, const uint8_t *, uint64_t, const uint64_t *, uint64_t, int, uint64_t *, uint64_t,
                        uint64_t *, uint64_t *, uint64_t *, uint64_t *);

int main(void) {
    frame_dev_fn frame_dev = nkv_frame_records_dev;
    frame_fn frame = nkv_frame_records;
    uint64_t n_out = 7, stats[4] = {7, 7, 7, 7};
    printf("abi %d\n", nkv_abi_version());
    printf("symbols %d\n", frame_dev != NULL && frame != NULL);
    printf("constants %d %d %d %d %d\n", NKV_FRAME_STRICT, NKV_OPT_FRAME_PATH, NKV_OPT_FRAME_BUDGET,
           NKV_PATH_FRAME_WALK, NKV_PATH_FRAME_SPECULATIVE);
    /* a null context is refused before anything else happens */
    printf("null_ctx %d %d\n",
           frame_dev(NULL, NULL, 0, NULL, 0, NKV_FRAME_STRICT, NULL, 0, NULL, NULL, &n_out, stats),
           frame(NULL, NULL, 0, NULL, 0, 0, NULL, 0, NULL, NULL, &n_out, stats));
    printf("untouched %d\n", n_out == 7 && stats[0] == 7 && stats[1] == 7 && stats[2] == 7 && stats[3] == 7);
    return 0;
}
