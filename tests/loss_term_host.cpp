// Host harness of csrc/yf_loss_term.h for tests/test_cpu_loss_hyp.py: reads records of 5 doubles (p, t, w, gamma, alpha) from argv[1],
// writes 2 doubles each (element, d element / d p) to argv[2].  The same function the kernel calls, compiled for the host.
#include <stdio.h>

#include "yf_loss_term.h"

int main(int argc, char** argv)
{
    if (argc != 3) return 2;
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!in || !out) return 3;
    double r[5], o[2];
    while (fread(r, sizeof(double), 5, in) == 5) {
        o[0] = yf::loss_elem(r[0], r[1], r[2], r[3], r[4], o + 1);
        if (fwrite(o, sizeof(double), 2, out) != 2) return 4;
    }
    fclose(in);
    return fclose(out) ? 5 : 0;
}
