/*
 * index_abi_c99.c -- the Index / Summary entry points as cgo sees them: built
 * with gcc -std=c99 -pedantic -Werror (tests/test_index_abi.py).  It takes the
 * addresses of the three entries through pointers of exactly the declared
 * types, prints the ABI version, the status a null context gets, and
 * nkv_summary_entries over the (n, page) pairs given on the command line.  No
 * device is touched.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "nkv_merkle.h"

typedef uint64_t (*entries_fn)(uint64_t, uint64_t);
typedef int (*index_dev_fn)(nkv_ctx *, const void *, uint64_t, const uint64_t *, uint64_t, uint64_t, void *,
                            uint64_t, void *, uint64_t, uint64_t *, uint64_t *);
typedef int (*index_host_fn)(nkv_ctx *, const uint8_t *, uint64_t, const uint64_t *, uint64_t, uint64_t,
                             uint8_t *, uint64_t, uint8_t *, uint64_t, uint64_t *, uint64_t *);

int main(int argc, char **argv) {
    entries_fn entries = nkv_summary_entries;
    index_dev_fn dev = nkv_index_summary_dev;
    index_host_fn host = nkv_index_summary_from_records;
    uint64_t index_len = 7, summary_len = 7;
    int i;
    printf("abi %d\n", nkv_abi_version());
    printf("symbols %d\n", entries != NULL && dev != NULL && host != NULL);
    /* a null context is refused before anything else happens */
    printf("null_ctx %d %d\n", dev(NULL, NULL, 0, NULL, 0, 3, NULL, 0, NULL, 0, &index_len, &summary_len),
           host(NULL, NULL, 0, NULL, 0, 3, NULL, 0, NULL, 0, &index_len, &summary_len));
    printf("entries");
    for (i = 1; i + 1 < argc; i += 2)
        printf(" %llu", (unsigned long long)entries(strtoull(argv[i], NULL, 10), strtoull(argv[i + 1], NULL, 10)));
    printf("\n");
    return 0;
}
