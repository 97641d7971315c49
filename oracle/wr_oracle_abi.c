/* The drop-in C ABI (setup_wr / encoding_wrap / decoding_wrap, include/waverange_amd.h) on the CPU oracle.
 *
 * TEST INFRASTRUCTURE ONLY (see wr_oracle.h): the command-line front-ends (waverange_amd/csrc/cli) link against it so that
 * their file formats and parameter handling are tested on a machine without a GPU and without the compiled reference
 * (tests/test_cli.py, tests/test_mssg.py, tests/test_sanitizers.py).  The oracle is pinned bit for bit to the reference
 * (tests/test_oracle_vs_ref.py), so the files the front-ends write on it are the reference CLI's. */
#include "wr_oracle.h"

void setup_wr(int nx, int ny, int nz, unsigned char *nlaymax, unsigned long *ntot_enc_max)
{
    wro_setup(nx, ny, nz, nlaymax, ntot_enc_max);
}

void encoding_wrap(int nx, int ny, int nz, double *fld_1d, int wtflag, int mx, int my, int mz,
                   double *cutoffvec, double *tolabs, double *midval, double *halfspanval,
                   unsigned char *wlev, unsigned char *nlay, unsigned long *ntot_enc,
                   double *deps_vec, double *minval_vec, unsigned long *len_enc_vec,
                   unsigned char *data_enc)
{
    wro_encode(nx, ny, nz, fld_1d, wtflag, mx, my, mz, cutoffvec, tolabs, midval, halfspanval, wlev, nlay, ntot_enc,
               deps_vec, minval_vec, len_enc_vec, data_enc);
}

void decoding_wrap(int nx, int ny, int nz, double *fld_1d, double *tolabs, double *midval,
                   double *halfspanval, unsigned char *wlev, unsigned char *nlay,
                   unsigned long *ntot_enc, double *deps_vec, double *minval_vec,
                   unsigned long *len_enc_vec, unsigned char *data_enc)
{
    (void)tolabs;
    (void)halfspanval;
    wro_decode(nx, ny, nz, fld_1d, *midval, *wlev, *nlay, *ntot_enc, deps_vec, minval_vec, len_enc_vec, data_enc);
}
