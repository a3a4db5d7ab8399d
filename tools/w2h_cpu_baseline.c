/* MEASUREMENT: times WordHyphenationWithModel of a blingfiretokdll-compatible library on host threads -- the yardstick of tools/bench_w2h.py.
 * The library is opened with dlopen (nothing of it is linked here); every thread calls the single-word entry point on its own contiguous slice
 * of the words, with an output buffer of its own.  Returns the seconds of one pass over all words (threads started .. joined), < 0 on error. */
#define _GNU_SOURCE
#include <dlfcn.h>
#include <pthread.h>
#include <stdint.h>
#include <stdlib.h>
#include <time.h>

typedef void *(*load_fn)(const char *);
typedef int (*free_fn)(void *);
typedef int (*hyph_fn)(const char *, int, char *, int, void *, int);

struct job { hyph_fn f; void *h; const char *text; const int64_t *off; int64_t lo, hi; int uhy; int64_t bytes, failed; };

static void *run(void *p)
{
    struct job *j = (struct job *)p;
    char out[4096];
    for (int64_t w = j->lo; w < j->hi; ++w) {
        const int r = j->f(j->text + j->off[w], (int)(j->off[w + 1] - j->off[w]), out, (int)sizeof out, j->h, j->uhy);
        if (r > 0) j->bytes += r - 1; else if (j->off[w + 1] > j->off[w]) ++j->failed;
    }
    return NULL;
}

static void *g_lib, *g_h;

int w2h_cpu_open(const char *lib, const char *model)
{
    g_lib = dlopen(lib, RTLD_NOW | RTLD_LOCAL);
    if (!g_lib) return -1;
    load_fn ld = (load_fn)dlsym(g_lib, "LoadModel");
    g_h = ld ? ld(model) : NULL;
    return g_h ? 0 : -2;
}

double w2h_cpu_pass(const char *text, const int64_t *off, int64_t n, int nthreads, int uhy, int64_t *bytes, int64_t *failed)
{
    hyph_fn f = g_lib ? (hyph_fn)dlsym(g_lib, "WordHyphenationWithModel") : NULL;
    if (!f || !g_h || nthreads < 1 || nthreads > 256) return -1.0;
    pthread_t th[256]; struct job jobs[256];
    struct timespec t0, t1;
    clock_gettime(CLOCK_MONOTONIC, &t0);
    for (int t = 0; t < nthreads; ++t) {
        jobs[t] = (struct job){f, g_h, text, off, n * t / nthreads, n * (t + 1) / nthreads, uhy, 0, 0};
        if (pthread_create(&th[t], NULL, run, &jobs[t]) != 0) return -2.0;
    }
    *bytes = 0; *failed = 0;
    for (int t = 0; t < nthreads; ++t) { pthread_join(th[t], NULL); *bytes += jobs[t].bytes; *failed += jobs[t].failed; }
    clock_gettime(CLOCK_MONOTONIC, &t1);
    return (double)(t1.tv_sec - t0.tv_sec) + 1e-9 * (double)(t1.tv_nsec - t0.tv_nsec);
}

void w2h_cpu_close(void)
{
    free_fn fr = g_lib ? (free_fn)dlsym(g_lib, "FreeModel") : NULL;
    if (fr && g_h) fr(g_h);
    g_h = NULL;
}
