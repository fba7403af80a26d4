/* How text that N producer threads have just formatted reaches one output
 * file fastest (gac_par_output's direct path).  The producers'
 * only work is filling their buffers; five schemes write the same bytes:
 *
 *   inorder   one writer thread writev()s the producers' runs in order, 256
 *             per call; every run freshly malloc'd by its producer and freed
 *             by the writer (the ordered writer of gac_par_output)
 *   own-run   each producer pwrite()s its own run at run * RUN
 *   own-group each producer fills a group of runs back to back in a buffer it
 *             reuses and pwrite()s it at group * GROUP
 *   own-var   the same with run lengths varying between RUN/2 and 3*RUN/2:
 *             a group's offset is known only when the groups before it have
 *             published their lengths (resolved in order, as the tool does)
 *   ceiling   one thread write()s a ready buffer of the whole size
 *
 * usage: own_group_write_probe DIR MB PRODUCERS RUN_BYTES GROUP_BYTES [REPS]
 * build: cc -O2 -pthread own_group_write_probe.c -o own_group_write_probe */
#define _GNU_SOURCE
#include <errno.h>
#include <fcntl.h>
#include <pthread.h>
#include <stdatomic.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/uio.h>
#include <sys/vfs.h>
#include <time.h>
#include <unistd.h>

static double now(void) {
    struct timespec t;
    clock_gettime(CLOCK_MONOTONIC, &t);
    return t.tv_sec + 1e-9 * t.tv_nsec;
}

static void die(const char *what) {
    perror(what);
    exit(1);
}

/* the producers' work: text-like bytes that depend on the position */
static void fill(char *p, size_t n, size_t seed) {
    for (size_t i = 0; i < n; ++i)
        p[i] = (char)('0' + (seed + i) % 43);
}

static void pwrite_all(int fd, const char *p, size_t n, off_t off) {
    while (n) {
        const ssize_t w = pwrite(fd, p, n, off);
        if (w < 0 && errno == EINTR)
            continue;
        if (w <= 0)
            die("pwrite");
        p += w;
        n -= (size_t)w;
        off += w;
    }
}

typedef struct job {
    int fd, scheme;
    size_t run, group, nruns, ngroups;
    _Atomic size_t next;
    char **buf;           /* inorder: the runs */
    _Atomic int *ready;   /* inorder */
    _Atomic int64_t *off; /* own-var: [ngroups + 1], -1 unknown */
    _Atomic int64_t *len; /* own-var: [ngroups], -1 unknown */
} job;

static size_t var_len(const job *J, size_t r) { /* RUN/2 .. 3*RUN/2 */
    return J->run / 2 + (r * 2654435761u) % (J->run + 1);
}

static int64_t var_offset(job *J, size_t g) {
    size_t k = g;
    int64_t o;
    while ((o = atomic_load_explicit(&J->off[k], memory_order_acquire)) < 0)
        --k;
    for (; k < g; ++k) {
        const int64_t l = atomic_load_explicit(&J->len[k], memory_order_acquire);
        if (l < 0)
            return -1;
        o += l;
        atomic_store_explicit(&J->off[k + 1], o, memory_order_release);
    }
    return o;
}

static void *producer(void *arg) {
    job *J = arg;
    const size_t per = J->group / J->run ? J->group / J->run : 1; /* runs per group */
    char *mine = NULL;
    size_t cap = 0;
    for (;;) {
        if (J->scheme == 0) { /* inorder: a fresh buffer per run, handed over */
            const size_t r = atomic_fetch_add(&J->next, 1);
            if (r >= J->nruns)
                break;
            char *p = malloc(J->run);
            fill(p, J->run, r);
            J->buf[r] = p;
            atomic_store_explicit(&J->ready[r], 1, memory_order_release);
        } else if (J->scheme == 1) { /* own-run */
            const size_t r = atomic_fetch_add(&J->next, 1);
            if (r >= J->nruns)
                break;
            if (!mine)
                mine = malloc(J->run);
            fill(mine, J->run, r);
            pwrite_all(J->fd, mine, J->run, (off_t)(r * J->run));
        } else if (J->scheme == 2) { /* own-group */
            const size_t g = atomic_fetch_add(&J->next, 1);
            if (g >= J->ngroups)
                break;
            const size_t r0 = g * per, r1 = r0 + per < J->nruns ? r0 + per : J->nruns;
            if (!mine)
                mine = malloc(per * J->run);
            for (size_t r = r0; r < r1; ++r)
                fill(mine + (r - r0) * J->run, J->run, r);
            pwrite_all(J->fd, mine, (r1 - r0) * J->run, (off_t)(r0 * J->run));
        } else { /* own-var */
            const size_t g = atomic_fetch_add(&J->next, 1);
            if (g >= J->ngroups)
                break;
            const size_t r0 = g * per, r1 = r0 + per < J->nruns ? r0 + per : J->nruns;
            size_t n = 0;
            for (size_t r = r0; r < r1; ++r) {
                const size_t l = var_len(J, r);
                if (n + l > cap) {
                    cap = 2 * (n + l);
                    mine = realloc(mine, cap);
                }
                fill(mine + n, l, r);
                n += l;
            }
            atomic_store_explicit(&J->len[g], (int64_t)n, memory_order_release);
            int64_t o;
            for (int spin = 0; (o = var_offset(J, g)) < 0; ++spin)
                if (spin >= 64)
                    usleep(20);
            pwrite_all(J->fd, mine, n, (off_t)o);
        }
    }
    free(mine);
    return NULL;
}

static void *inorder_writer(void *arg) {
    job *J = arg;
    size_t r = 0;
    while (r < J->nruns) {
        struct iovec iov[256];
        int k = 0;
        const size_t r0 = r;
        while (!atomic_load_explicit(&J->ready[r], memory_order_acquire))
            __builtin_ia32_pause();
        while (r < J->nruns && k < 256 &&
               (r == r0 || atomic_load_explicit(&J->ready[r], memory_order_acquire))) {
            iov[k].iov_base = J->buf[r];
            iov[k].iov_len = J->run;
            ++k;
            ++r;
        }
        struct iovec *v = iov;
        while (k > 0) {
            ssize_t w = writev(J->fd, v, k);
            if (w < 0 && errno == EINTR)
                continue;
            if (w <= 0)
                die("writev");
            while (k > 0 && (size_t)w >= v->iov_len) {
                w -= (ssize_t)v->iov_len;
                ++v;
                --k;
            }
            if (k > 0) {
                v->iov_base = (char *)v->iov_base + w;
                v->iov_len -= (size_t)w;
            }
        }
        for (size_t x = r0; x < r; ++x)
            free(J->buf[x]);
    }
    return NULL;
}

int main(int argc, char **argv) {
    if (argc < 6) {
        fprintf(stderr, "usage: %s DIR MB PRODUCERS RUN_BYTES GROUP_BYTES [REPS]\n", argv[0]);
        return 2;
    }
    const char *dir = argv[1];
    const size_t size = (size_t)atol(argv[2]) << 20;
    int np = atoi(argv[3]);
    const size_t run = (size_t)atol(argv[4]), group = (size_t)atol(argv[5]);
    const int reps = argc > 6 ? atoi(argv[6]) : 2;
    if (np < 1 || np > 256 || run < 16 || group < run || size < group) {
        fprintf(stderr, "bad arguments\n");
        return 2;
    }
    char path[4096];
    snprintf(path, sizeof path, "%s/own_group_write_probe.out", dir);
    struct statfs sf;
    if (statfs(dir, &sf) == 0)
        printf("fs magic 0x%lx, %zu MB, %d producers, run %zu, group %zu\n", (long)sf.f_type,
               size >> 20, np, run, group);
    static const char *const name[5] = {"inorder", "own-run", "own-group", "own-var", "ceiling"};
    job J;
    memset(&J, 0, sizeof J);
    J.run = run;
    J.group = group;
    J.nruns = size / run;
    const size_t per = group / run;
    J.ngroups = (J.nruns + per - 1) / per;
    J.buf = calloc(J.nruns, sizeof(char *));
    J.ready = calloc(J.nruns, sizeof(_Atomic int));
    J.off = malloc((J.ngroups + 1) * sizeof(*J.off));
    J.len = malloc(J.ngroups * sizeof(*J.len));
    char *whole = malloc(size);
    fill(whole, size, 7);
    pthread_t *th = malloc((size_t)(np + 1) * sizeof(pthread_t));
    for (int rep = 0; rep < reps; ++rep)
        for (int s = 0; s < 5; ++s) {
            unlink(path);
            const int fd = open(path, O_WRONLY | O_CREAT | O_TRUNC, 0644);
            if (fd < 0)
                die(path);
            J.fd = fd;
            J.scheme = s;
            atomic_store(&J.next, 0);
            for (size_t r = 0; r < J.nruns; ++r)
                atomic_store(&J.ready[r], 0);
            for (size_t g = 0; g < J.ngroups; ++g) {
                atomic_store(&J.off[g + 1], -1);
                atomic_store(&J.len[g], -1);
            }
            atomic_store(&J.off[0], 0);
            size_t bytes = J.nruns * run;
            const double t0 = now();
            if (s == 4) {
                bytes = size;
                for (size_t d = 0; d < size;) {
                    const size_t n = size - d < (8u << 20) ? size - d : (8u << 20);
                    const ssize_t w = write(fd, whole + d, n);
                    if (w <= 0)
                        die("write");
                    d += (size_t)w;
                }
            } else {
                for (int i = 0; i < np; ++i)
                    pthread_create(&th[i], NULL, producer, &J);
                if (s == 0)
                    pthread_create(&th[np], NULL, inorder_writer, &J);
                for (int i = 0; i < np + (s == 0); ++i)
                    pthread_join(th[i], NULL);
                if (s == 3)
                    bytes = (size_t)var_offset(&J, J.ngroups);
            }
            const double t1 = now();
            const off_t end = lseek(fd, 0, SEEK_END);
            close(fd);
            printf("rep %d %-9s %.3f s  %.2f GB/s  (%zu bytes, file %lld)\n", rep, name[s], t1 - t0,
                   (double)bytes / (t1 - t0) / 1e9, bytes, (long long)end);
            fflush(stdout);
        }
    unlink(path);
    return 0;
}
