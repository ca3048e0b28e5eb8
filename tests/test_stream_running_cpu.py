"""CPU-only checks of running preintegration from IMU stream(s) (cpi_preintegrate_stream_running / _streams_running and their
_host forms): the symbols are declared, listed under "additions within 3" and exported, the Python layer knows them, a NULL
context is refused, the new kernels stand in the build report without scratch, and every row the report held before this
feature -- registers, LDS, scratch, occupancy of every kernel -- is still there unchanged."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("cpi_preintegrate_stream_running", "cpi_preintegrate_streams_running", "cpi_preintegrate_stream_running_host",
           "cpi_preintegrate_streams_running_host")

# cpi_amd/csrc/resource_usage.txt as it stood before cpi_mean_stream_running_kernel existed (header line left out)
PARENT_ROWS = """\
cpi_tile_knots_kernel                                                       51    22     0       0    8      0
cpi_cut_windows_kernel                                                      48    26     0       0    8      0
cpi_cut_runs_kernel                                                         44    36     0       0    8      0
cpi_assemble_tiles_kernel                                                   69   138     0       0    1  33536
cpi_mean_kernel<2, true, true, 1, 1, false>                                106   256   154       0    1   4096
cpi_mean_kernel<2, true, true, 1, 0, false>                                100   256   158       0    1   4096
cpi_mean_kernel<2, true, false, 1, 1, false>                               106   256   156       0    1   4096
cpi_mean_kernel<2, true, false, 1, 0, false>                               100   256   162       0    1   4096
cpi_mean_kernel<2, false, true, 1, 2, true>                                 89   224     0       0    2  11264
cpi_mean_kernel<2, false, true, 1, 1, true>                                 89   226     0       0    2  11264
cpi_mean_kernel<2, false, true, 1, 0, true>                                 81   222     0       0    2  11264
cpi_mean_kernel<2, false, true, 1, 2, false>                                87   238     0       0    2   8192
cpi_mean_kernel<2, false, true, 1, 1, false>                                87   240     0       0    2   8192
cpi_mean_kernel<2, false, true, 1, 0, false>                                79   236     0       0    2   8192
cpi_mean_kernel<2, false, true, 2, 2, false>                                93   256    50       0    1   8192
cpi_mean_kernel<2, false, true, 2, 1, false>                                93   256    52       0    1   8192
cpi_mean_kernel<2, false, true, 2, 0, false>                                85   256    50       0    1   8192
cpi_mean_kernel<2, false, true, 3, 2, false>                                93   256    50       0    1   8192
cpi_mean_kernel<2, false, true, 3, 1, false>                                93   256    54       0    1   8192
cpi_mean_kernel<2, false, true, 3, 0, false>                                85   256    52       0    1   8192
cpi_mean_kernel<2, false, true, 4, 2, false>                                93   256    50       0    1   8192
cpi_mean_kernel<2, false, true, 4, 1, false>                                93   256    52       0    1   8192
cpi_mean_kernel<2, false, true, 4, 0, false>                                85   256    50       0    1   8192
cpi_mean_kernel<2, false, true, 5, 2, false>                                93   256    50       0    1   8192
cpi_mean_kernel<2, false, true, 5, 1, false>                                93   256    54       0    1   8192
cpi_mean_kernel<2, false, true, 5, 0, false>                                85   256    52       0    1   8192
cpi_mean_kernel<2, false, true, 6, 2, false>                                93   256    50       0    1   8192
cpi_mean_kernel<2, false, true, 6, 1, false>                                93   256    54       0    1   8192
cpi_mean_kernel<2, false, true, 6, 0, false>                                85   256    52       0    1   8192
cpi_mean_kernel<2, false, true, 8, 2, false>                                93   256    50       0    1   8192
cpi_mean_kernel<2, false, true, 8, 1, false>                                93   256    52       0    1   8192
cpi_mean_kernel<2, false, true, 8, 0, false>                                85   256    50       0    1   8192
cpi_mean_kernel<2, false, true, 12, 2, false>                               88   246     0       0    2   4096
cpi_mean_kernel<2, false, true, 12, 1, false>                               88   248     0       0    2   4096
cpi_mean_kernel<2, false, true, 12, 0, false>                               82   246     0       0    2   4096
cpi_mean_kernel<2, false, true, 16, 2, false>                               88   244     0       0    2   4096
cpi_mean_kernel<2, false, true, 16, 1, false>                               88   248     0       0    2   4096
cpi_mean_kernel<2, false, true, 16, 0, false>                               82   244     0       0    2   4096
cpi_mean_kernel<2, false, true, 32, 2, false>                               88   244     0       0    2   4096
cpi_mean_kernel<2, false, true, 32, 1, false>                               88   248     0       0    2   4096
cpi_mean_kernel<2, false, true, 32, 0, false>                               82   244     0       0    2   4096
cpi_mean_kernel<2, false, true, 64, 2, false>                               92   244     0       0    2   4096
cpi_mean_kernel<2, false, true, 64, 1, false>                               92   246     0       0    2   4096
cpi_mean_kernel<2, false, true, 64, 0, false>                               86   242     0       0    2   4096
cpi_mean_kernel<2, false, false, 1, 2, true>                                89   218     0       0    2  11264
cpi_mean_kernel<2, false, false, 1, 1, true>                                89   220     0       0    2  11264
cpi_mean_kernel<2, false, false, 1, 0, true>                                81   216     0       0    2  11264
cpi_mean_kernel<2, false, false, 1, 2, false>                               87   232     0       0    2   8192
cpi_mean_kernel<2, false, false, 1, 1, false>                               87   234     0       0    2   8192
cpi_mean_kernel<2, false, false, 1, 0, false>                               79   230     0       0    2   8192
cpi_mean_kernel<2, false, false, 2, 2, false>                               93   256    52       0    1   8192
cpi_mean_kernel<2, false, false, 2, 1, false>                               93   256    54       0    1   8192
cpi_mean_kernel<2, false, false, 2, 0, false>                               85   256    52       0    1   8192
cpi_mean_kernel<2, false, false, 3, 2, false>                               93   256    52       0    1   8192
cpi_mean_kernel<2, false, false, 3, 1, false>                               93   256    56       0    1   8192
cpi_mean_kernel<2, false, false, 3, 0, false>                               85   256    54       0    1   8192
cpi_mean_kernel<2, false, false, 4, 2, false>                               93   256    52       0    1   8192
cpi_mean_kernel<2, false, false, 4, 1, false>                               93   256    54       0    1   8192
cpi_mean_kernel<2, false, false, 4, 0, false>                               85   256    52       0    1   8192
cpi_mean_kernel<2, false, false, 5, 2, false>                               93   256    52       0    1   8192
cpi_mean_kernel<2, false, false, 5, 1, false>                               93   256    56       0    1   8192
cpi_mean_kernel<2, false, false, 5, 0, false>                               85   256    54       0    1   8192
cpi_mean_kernel<2, false, false, 6, 2, false>                               93   256    52       0    1   8192
cpi_mean_kernel<2, false, false, 6, 1, false>                               93   256    56       0    1   8192
cpi_mean_kernel<2, false, false, 6, 0, false>                               85   256    54       0    1   8192
cpi_mean_kernel<2, false, false, 8, 2, false>                               93   256    52       0    1   8192
cpi_mean_kernel<2, false, false, 8, 1, false>                               93   256    54       0    1   8192
cpi_mean_kernel<2, false, false, 8, 0, false>                               85   256    52       0    1   8192
cpi_mean_kernel<2, false, false, 12, 2, false>                              88   256     4       0    1   4096
cpi_mean_kernel<2, false, false, 12, 1, false>                              88   256    10       0    1   4096
cpi_mean_kernel<2, false, false, 12, 0, false>                              82   256     6       0    1   4096
cpi_mean_kernel<2, false, false, 16, 2, false>                              88   256     4       0    1   4096
cpi_mean_kernel<2, false, false, 16, 1, false>                              88   256     8       0    1   4096
cpi_mean_kernel<2, false, false, 16, 0, false>                              82   256     4       0    1   4096
cpi_mean_kernel<2, false, false, 32, 2, false>                              88   256     4       0    1   4096
cpi_mean_kernel<2, false, false, 32, 1, false>                              88   256     8       0    1   4096
cpi_mean_kernel<2, false, false, 32, 0, false>                              82   256     4       0    1   4096
cpi_mean_kernel<2, false, false, 64, 2, false>                              92   256     2       0    1   4096
cpi_mean_kernel<2, false, false, 64, 1, false>                              92   256     4       0    1   4096
cpi_mean_kernel<2, false, false, 64, 0, false>                              86   256     0       0    2   4096
cpi_mean_kernel<1, true, true, 1, 1, false>                                 94   256     0      52    2      0
cpi_mean_kernel<1, true, true, 1, 0, false>                                 92   256     0      36    2      0
cpi_mean_kernel<1, true, true, 2, 1, false>                                102   256    46       0    1   4096
cpi_mean_kernel<1, true, true, 2, 0, false>                                 96   256    44       0    1   4096
cpi_mean_kernel<1, true, true, 3, 1, false>                                102   256    48       0    1   4096
cpi_mean_kernel<1, true, true, 3, 0, false>                                 96   256    46       0    1   4096
cpi_mean_kernel<1, true, true, 4, 1, false>                                102   256    46       0    1   4096
cpi_mean_kernel<1, true, true, 4, 0, false>                                 96   256    44       0    1   4096
cpi_mean_kernel<1, true, true, 5, 1, false>                                102   256    48       0    1   4096
cpi_mean_kernel<1, true, true, 5, 0, false>                                 96   256    46       0    1   4096
cpi_mean_kernel<1, true, true, 6, 1, false>                                102   256    48       0    1   4096
cpi_mean_kernel<1, true, true, 6, 0, false>                                 96   256    46       0    1   4096
cpi_mean_kernel<1, true, true, 8, 1, false>                                102   256    46       0    1   4096
cpi_mean_kernel<1, true, true, 8, 0, false>                                 96   256    44       0    1   4096
cpi_mean_kernel<1, true, true, 12, 1, false>                               102   256    48       0    1   4096
cpi_mean_kernel<1, true, true, 12, 0, false>                                96   256    46       0    1   4096
cpi_mean_kernel<1, true, true, 16, 1, false>                               102   256    46       0    1   4096
cpi_mean_kernel<1, true, true, 16, 0, false>                                96   256    44       0    1   4096
cpi_mean_kernel<1, true, true, 32, 1, false>                               102   256    46       0    1   4096
cpi_mean_kernel<1, true, true, 32, 0, false>                                96   256    44       0    1   4096
cpi_mean_kernel<1, true, true, 64, 1, false>                               106   256    44       0    1   4096
cpi_mean_kernel<1, true, true, 64, 0, false>                               100   256    42       0    1   4096
cpi_mean_kernel<1, true, false, 1, 1, false>                                96   256     0      76    2      0
cpi_mean_kernel<1, true, false, 1, 0, false>                                92   256     0      36    2      0
cpi_mean_kernel<1, true, false, 2, 1, false>                               102   256    46       0    1   4096
cpi_mean_kernel<1, true, false, 2, 0, false>                                96   256    44       0    1   4096
cpi_mean_kernel<1, true, false, 3, 1, false>                               102   256    48       0    1   4096
cpi_mean_kernel<1, true, false, 3, 0, false>                                96   256    46       0    1   4096
cpi_mean_kernel<1, true, false, 4, 1, false>                               102   256    46       0    1   4096
cpi_mean_kernel<1, true, false, 4, 0, false>                                96   256    44       0    1   4096
cpi_mean_kernel<1, true, false, 5, 1, false>                               102   256    48       0    1   4096
cpi_mean_kernel<1, true, false, 5, 0, false>                                96   256    46       0    1   4096
cpi_mean_kernel<1, true, false, 6, 1, false>                               102   256    48       0    1   4096
cpi_mean_kernel<1, true, false, 6, 0, false>                                96   256    46       0    1   4096
cpi_mean_kernel<1, true, false, 8, 1, false>                               102   256    46       0    1   4096
cpi_mean_kernel<1, true, false, 8, 0, false>                                96   256    44       0    1   4096
cpi_mean_kernel<1, true, false, 12, 1, false>                              102   256    48       0    1   4096
cpi_mean_kernel<1, true, false, 12, 0, false>                               96   256    46       0    1   4096
cpi_mean_kernel<1, true, false, 16, 1, false>                              102   256    46       0    1   4096
cpi_mean_kernel<1, true, false, 16, 0, false>                               96   256    44       0    1   4096
cpi_mean_kernel<1, true, false, 32, 1, false>                              102   256    46       0    1   4096
cpi_mean_kernel<1, true, false, 32, 0, false>                               96   256    44       0    1   4096
cpi_mean_kernel<1, true, false, 64, 1, false>                              106   256    44       0    1   4096
cpi_mean_kernel<1, true, false, 64, 0, false>                              100   256    42       0    1   4096
cpi_mean_kernel<1, false, true, 1, 2, true>                                 89   208     0       0    2  11264
cpi_mean_kernel<1, false, true, 1, 1, true>                                 89   210     0       0    2  11264
cpi_mean_kernel<1, false, true, 1, 0, true>                                 81   208     0       0    2  11264
cpi_mean_kernel<1, false, true, 1, 2, false>                                87   222     0       0    2   8192
cpi_mean_kernel<1, false, true, 1, 1, false>                                87   224     0       0    2   8192
cpi_mean_kernel<1, false, true, 1, 0, false>                                79   222     0       0    2   8192
cpi_mean_kernel<1, false, true, 2, 2, false>                                87   222     0       0    2   8192
cpi_mean_kernel<1, false, true, 2, 1, false>                                87   224     0       0    2   8192
cpi_mean_kernel<1, false, true, 2, 0, false>                                79   222     0       0    2   8192
cpi_mean_kernel<1, false, true, 3, 2, false>                                87   222     0       0    2   8192
cpi_mean_kernel<1, false, true, 3, 1, false>                                87   226     0       0    2   8192
cpi_mean_kernel<1, false, true, 3, 0, false>                                79   224     0       0    2   8192
cpi_mean_kernel<1, false, true, 4, 2, false>                                87   222     0       0    2   8192
cpi_mean_kernel<1, false, true, 4, 1, false>                                87   224     0       0    2   8192
cpi_mean_kernel<1, false, true, 4, 0, false>                                79   222     0       0    2   8192
cpi_mean_kernel<1, false, true, 5, 2, false>                                87   222     0       0    2   8192
cpi_mean_kernel<1, false, true, 5, 1, false>                                87   226     0       0    2   8192
cpi_mean_kernel<1, false, true, 5, 0, false>                                79   224     0       0    2   8192
cpi_mean_kernel<1, false, true, 6, 2, false>                                87   222     0       0    2   8192
cpi_mean_kernel<1, false, true, 6, 1, false>                                87   226     0       0    2   8192
cpi_mean_kernel<1, false, true, 6, 0, false>                                79   224     0       0    2   8192
cpi_mean_kernel<1, false, true, 8, 2, false>                                87   222     0       0    2   8192
cpi_mean_kernel<1, false, true, 8, 1, false>                                87   224     0       0    2   8192
cpi_mean_kernel<1, false, true, 8, 0, false>                                79   222     0       0    2   8192
cpi_mean_kernel<1, false, true, 12, 2, false>                               82   164     0       0    3   4096
cpi_mean_kernel<1, false, true, 12, 1, false>                               82   166     0       0    3   4096
cpi_mean_kernel<1, false, true, 12, 0, false>                               76   164     0       0    3   4096
cpi_mean_kernel<1, false, true, 16, 2, false>                               82   162     0       0    3   4096
cpi_mean_kernel<1, false, true, 16, 1, false>                               82   166     0       0    3   4096
cpi_mean_kernel<1, false, true, 16, 0, false>                               76   162     0       0    3   4096
cpi_mean_kernel<1, false, true, 32, 2, false>                               82   162     0       0    3   4096
cpi_mean_kernel<1, false, true, 32, 1, false>                               82   166     0       0    3   4096
cpi_mean_kernel<1, false, true, 32, 0, false>                               76   162     0       0    3   4096
cpi_mean_kernel<1, false, true, 64, 2, false>                               86   162     0       0    3   4096
cpi_mean_kernel<1, false, true, 64, 1, false>                               86   164     0       0    3   4096
cpi_mean_kernel<1, false, true, 64, 0, false>                               80   160     0       0    3   4096
cpi_mean_kernel<1, false, false, 1, 2, true>                                89   200     0       0    2  11264
cpi_mean_kernel<1, false, false, 1, 1, true>                                89   202     0       0    2  11264
cpi_mean_kernel<1, false, false, 1, 0, true>                                81   198     0       0    2  11264
cpi_mean_kernel<1, false, false, 1, 2, false>                               87   214     0       0    2   8192
cpi_mean_kernel<1, false, false, 1, 1, false>                               87   216     0       0    2   8192
cpi_mean_kernel<1, false, false, 1, 0, false>                               79   212     0       0    2   8192
cpi_mean_kernel<1, false, false, 2, 2, false>                               87   214     0       0    2   8192
cpi_mean_kernel<1, false, false, 2, 1, false>                               87   216     0       0    2   8192
cpi_mean_kernel<1, false, false, 2, 0, false>                               79   212     0       0    2   8192
cpi_mean_kernel<1, false, false, 3, 2, false>                               87   214     0       0    2   8192
cpi_mean_kernel<1, false, false, 3, 1, false>                               87   218     0       0    2   8192
cpi_mean_kernel<1, false, false, 3, 0, false>                               79   214     0       0    2   8192
cpi_mean_kernel<1, false, false, 4, 2, false>                               87   214     0       0    2   8192
cpi_mean_kernel<1, false, false, 4, 1, false>                               87   216     0       0    2   8192
cpi_mean_kernel<1, false, false, 4, 0, false>                               79   212     0       0    2   8192
cpi_mean_kernel<1, false, false, 5, 2, false>                               87   214     0       0    2   8192
cpi_mean_kernel<1, false, false, 5, 1, false>                               87   218     0       0    2   8192
cpi_mean_kernel<1, false, false, 5, 0, false>                               79   214     0       0    2   8192
cpi_mean_kernel<1, false, false, 6, 2, false>                               87   214     0       0    2   8192
cpi_mean_kernel<1, false, false, 6, 1, false>                               87   218     0       0    2   8192
cpi_mean_kernel<1, false, false, 6, 0, false>                               79   214     0       0    2   8192
cpi_mean_kernel<1, false, false, 8, 2, false>                               87   214     0       0    2   8192
cpi_mean_kernel<1, false, false, 8, 1, false>                               87   216     0       0    2   8192
cpi_mean_kernel<1, false, false, 8, 0, false>                               79   212     0       0    2   8192
cpi_mean_kernel<1, false, false, 12, 2, false>                              82   164     0       0    3   4096
cpi_mean_kernel<1, false, false, 12, 1, false>                              82   166     0       0    3   4096
cpi_mean_kernel<1, false, false, 12, 0, false>                              76   164     0       0    3   4096
cpi_mean_kernel<1, false, false, 16, 2, false>                              82   162     0       0    3   4096
cpi_mean_kernel<1, false, false, 16, 1, false>                              82   166     0       0    3   4096
cpi_mean_kernel<1, false, false, 16, 0, false>                              76   162     0       0    3   4096
cpi_mean_kernel<1, false, false, 32, 2, false>                              82   162     0       0    3   4096
cpi_mean_kernel<1, false, false, 32, 1, false>                              82   166     0       0    3   4096
cpi_mean_kernel<1, false, false, 32, 0, false>                              76   162     0       0    3   4096
cpi_mean_kernel<1, false, false, 64, 2, false>                              86   162     0       0    3   4096
cpi_mean_kernel<1, false, false, 64, 1, false>                              86   164     0       0    3   4096
cpi_mean_kernel<1, false, false, 64, 0, false>                              80   160     0       0    3   4096
cpi_mean_runs_kernel<2, true, 1, true>                                      96   224     0       0    2  11264
cpi_mean_runs_kernel<2, true, 1, false>                                     94   238     0       0    2   8192
cpi_mean_runs_kernel<2, true, 2, false>                                    100   256    50       0    1   8192
cpi_mean_runs_kernel<2, true, 3, false>                                    100   256    50       0    1   8192
cpi_mean_runs_kernel<2, true, 4, false>                                    100   256    50       0    1   8192
cpi_mean_runs_kernel<2, true, 5, false>                                    100   256    50       0    1   8192
cpi_mean_runs_kernel<2, true, 6, false>                                    100   256    50       0    1   8192
cpi_mean_runs_kernel<2, true, 8, false>                                    100   256    50       0    1   8192
cpi_mean_runs_kernel<2, true, 12, false>                                    95   246     0       0    2   4096
cpi_mean_runs_kernel<2, true, 16, false>                                    95   244     0       0    2   4096
cpi_mean_runs_kernel<2, true, 32, false>                                    95   244     0       0    2   4096
cpi_mean_runs_kernel<2, true, 64, false>                                    97   244     0       0    2   4096
cpi_mean_runs_kernel<2, false, 1, true>                                     96   218     0       0    2  11264
cpi_mean_runs_kernel<2, false, 1, false>                                    94   232     0       0    2   8192
cpi_mean_runs_kernel<2, false, 2, false>                                   100   256    52       0    1   8192
cpi_mean_runs_kernel<2, false, 3, false>                                   100   256    52       0    1   8192
cpi_mean_runs_kernel<2, false, 4, false>                                   100   256    52       0    1   8192
cpi_mean_runs_kernel<2, false, 5, false>                                   100   256    52       0    1   8192
cpi_mean_runs_kernel<2, false, 6, false>                                   100   256    52       0    1   8192
cpi_mean_runs_kernel<2, false, 8, false>                                   100   256    52       0    1   8192
cpi_mean_runs_kernel<2, false, 12, false>                                   95   256     4       0    1   4096
cpi_mean_runs_kernel<2, false, 16, false>                                   95   256     4       0    1   4096
cpi_mean_runs_kernel<2, false, 32, false>                                   95   256     4       0    1   4096
cpi_mean_runs_kernel<2, false, 64, false>                                   97   256     4       0    1   4096
cpi_mean_runs_kernel<1, true, 1, true>                                      96   208     0       0    2  11264
cpi_mean_runs_kernel<1, true, 1, false>                                     94   222     0       0    2   8192
cpi_mean_runs_kernel<1, true, 2, false>                                     94   222     0       0    2   8192
cpi_mean_runs_kernel<1, true, 3, false>                                     94   222     0       0    2   8192
cpi_mean_runs_kernel<1, true, 4, false>                                     94   222     0       0    2   8192
cpi_mean_runs_kernel<1, true, 5, false>                                     94   222     0       0    2   8192
cpi_mean_runs_kernel<1, true, 6, false>                                     94   222     0       0    2   8192
cpi_mean_runs_kernel<1, true, 8, false>                                     94   222     0       0    2   8192
cpi_mean_runs_kernel<1, true, 12, false>                                    89   164     0       0    3   4096
cpi_mean_runs_kernel<1, true, 16, false>                                    89   162     0       0    3   4096
cpi_mean_runs_kernel<1, true, 32, false>                                    89   162     0       0    3   4096
cpi_mean_runs_kernel<1, true, 64, false>                                    91   162     0       0    3   4096
cpi_mean_runs_kernel<1, false, 1, true>                                     96   200     0       0    2  11264
cpi_mean_runs_kernel<1, false, 1, false>                                    94   214     0       0    2   8192
cpi_mean_runs_kernel<1, false, 2, false>                                    94   214     0       0    2   8192
cpi_mean_runs_kernel<1, false, 3, false>                                    94   214     0       0    2   8192
cpi_mean_runs_kernel<1, false, 4, false>                                    94   214     0       0    2   8192
cpi_mean_runs_kernel<1, false, 5, false>                                    94   214     0       0    2   8192
cpi_mean_runs_kernel<1, false, 6, false>                                    94   214     0       0    2   8192
cpi_mean_runs_kernel<1, false, 8, false>                                    94   214     0       0    2   8192
cpi_mean_runs_kernel<1, false, 12, false>                                   89   164     0       0    3   4096
cpi_mean_runs_kernel<1, false, 16, false>                                   89   162     0       0    3   4096
cpi_mean_runs_kernel<1, false, 32, false>                                   89   162     0       0    3   4096
cpi_mean_runs_kernel<1, false, 64, false>                                   91   162     0       0    3   4096
cpi_mean_carry_kernel<2, true, true, 1>                                    106   256   156       0    1   4096
cpi_mean_carry_kernel<2, true, false, 1>                                   106   256   150       0    1   4096
cpi_mean_carry_kernel<2, false, true, 1>                                    85   236     0       0    2   8192
cpi_mean_carry_kernel<2, false, true, 2>                                    91   256    50       0    1   8192
cpi_mean_carry_kernel<2, false, true, 3>                                    91   256    52       0    1   8192
cpi_mean_carry_kernel<2, false, true, 4>                                    91   256    50       0    1   8192
cpi_mean_carry_kernel<2, false, true, 5>                                    91   256    52       0    1   8192
cpi_mean_carry_kernel<2, false, true, 6>                                    91   256    52       0    1   8192
cpi_mean_carry_kernel<2, false, true, 8>                                    91   256    50       0    1   8192
cpi_mean_carry_kernel<2, false, true, 12>                                   88   246     0       0    2   4096
cpi_mean_carry_kernel<2, false, true, 16>                                   88   244     0       0    2   4096
cpi_mean_carry_kernel<2, false, true, 32>                                   88   244     0       0    2   4096
cpi_mean_carry_kernel<2, false, true, 64>                                   92   242     0       0    2   4096
cpi_mean_carry_kernel<2, false, false, 1>                                   85   230     0       0    2   8192
cpi_mean_carry_kernel<2, false, false, 2>                                   91   256    52       0    1   8192
cpi_mean_carry_kernel<2, false, false, 3>                                   91   256    54       0    1   8192
cpi_mean_carry_kernel<2, false, false, 4>                                   91   256    52       0    1   8192
cpi_mean_carry_kernel<2, false, false, 5>                                   91   256    54       0    1   8192
cpi_mean_carry_kernel<2, false, false, 6>                                   91   256    54       0    1   8192
cpi_mean_carry_kernel<2, false, false, 8>                                   91   256    52       0    1   8192
cpi_mean_carry_kernel<2, false, false, 12>                                  88   256     6       0    1   4096
cpi_mean_carry_kernel<2, false, false, 16>                                  88   256     2       0    1   4096
cpi_mean_carry_kernel<2, false, false, 32>                                  88   256     2       0    1   4096
cpi_mean_carry_kernel<2, false, false, 64>                                  92   256     0       0    2   4096
cpi_mean_carry_kernel<1, true, true, 1>                                     98   256     0      36    2      0
cpi_mean_carry_kernel<1, true, true, 2>                                    102   256    44       0    1   4096
cpi_mean_carry_kernel<1, true, true, 3>                                    102   256    46       0    1   4096
cpi_mean_carry_kernel<1, true, true, 4>                                    102   256    44       0    1   4096
cpi_mean_carry_kernel<1, true, true, 5>                                    102   256    46       0    1   4096
cpi_mean_carry_kernel<1, true, true, 6>                                    102   256    46       0    1   4096
cpi_mean_carry_kernel<1, true, true, 8>                                    102   256    44       0    1   4096
cpi_mean_carry_kernel<1, true, true, 12>                                   102   256    46       0    1   4096
cpi_mean_carry_kernel<1, true, true, 16>                                   102   256    44       0    1   4096
cpi_mean_carry_kernel<1, true, true, 32>                                   102   256    44       0    1   4096
cpi_mean_carry_kernel<1, true, true, 64>                                   106   256    42       0    1   4096
cpi_mean_carry_kernel<1, true, false, 1>                                    98   256     0      36    2      0
cpi_mean_carry_kernel<1, true, false, 2>                                   102   256    44       0    1   4096
cpi_mean_carry_kernel<1, true, false, 3>                                   102   256    46       0    1   4096
cpi_mean_carry_kernel<1, true, false, 4>                                   102   256    44       0    1   4096
cpi_mean_carry_kernel<1, true, false, 5>                                   102   256    46       0    1   4096
cpi_mean_carry_kernel<1, true, false, 6>                                   102   256    46       0    1   4096
cpi_mean_carry_kernel<1, true, false, 8>                                   102   256    44       0    1   4096
cpi_mean_carry_kernel<1, true, false, 12>                                  102   256    46       0    1   4096
cpi_mean_carry_kernel<1, true, false, 16>                                  102   256    44       0    1   4096
cpi_mean_carry_kernel<1, true, false, 32>                                  102   256    46       0    1   4096
cpi_mean_carry_kernel<1, true, false, 64>                                  106   256    44       0    1   4096
cpi_mean_carry_kernel<1, false, true, 1>                                    85   222     0       0    2   8192
cpi_mean_carry_kernel<1, false, true, 2>                                    85   222     0       0    2   8192
cpi_mean_carry_kernel<1, false, true, 3>                                    85   224     0       0    2   8192
cpi_mean_carry_kernel<1, false, true, 4>                                    85   222     0       0    2   8192
cpi_mean_carry_kernel<1, false, true, 5>                                    85   224     0       0    2   8192
cpi_mean_carry_kernel<1, false, true, 6>                                    85   224     0       0    2   8192
cpi_mean_carry_kernel<1, false, true, 8>                                    85   222     0       0    2   8192
cpi_mean_carry_kernel<1, false, true, 12>                                   82   164     0       0    3   4096
cpi_mean_carry_kernel<1, false, true, 16>                                   82   162     0       0    3   4096
cpi_mean_carry_kernel<1, false, true, 32>                                   82   162     0       0    3   4096
cpi_mean_carry_kernel<1, false, true, 64>                                   86   160     0       0    3   4096
cpi_mean_carry_kernel<1, false, false, 1>                                   85   212     0       0    2   8192
cpi_mean_carry_kernel<1, false, false, 2>                                   85   212     0       0    2   8192
cpi_mean_carry_kernel<1, false, false, 3>                                   85   214     0       0    2   8192
cpi_mean_carry_kernel<1, false, false, 4>                                   85   212     0       0    2   8192
cpi_mean_carry_kernel<1, false, false, 5>                                   85   214     0       0    2   8192
cpi_mean_carry_kernel<1, false, false, 6>                                   85   214     0       0    2   8192
cpi_mean_carry_kernel<1, false, false, 8>                                   85   212     0       0    2   8192
cpi_mean_carry_kernel<1, false, false, 12>                                  82   164     0       0    3   4096
cpi_mean_carry_kernel<1, false, false, 16>                                  82   162     0       0    3   4096
cpi_mean_carry_kernel<1, false, false, 32>                                  82   162     0       0    3   4096
cpi_mean_carry_kernel<1, false, false, 64>                                  86   160     0       0    3   4096
cpi_mean_tiled_kernel<1, true, true, true>                                  77   156     0       0    3      0
cpi_mean_tiled_kernel<1, true, true, false>                                 75   152     0       0    3      0
cpi_mean_tiled_kernel<1, false, true, true>                                 77   156     0       0    3      0
cpi_mean_tiled_kernel<1, false, true, false>                                75   152     0       0    3      0
cpi_mean_tiled_kernel<1, true, false, true>                                 78   156     0       0    3      0
cpi_mean_tiled_kernel<1, true, false, false>                                76   150     0       0    3      0
cpi_mean_tiled_kernel<1, false, false, true>                                78   156     0       0    3      0
cpi_mean_tiled_kernel<1, false, false, false>                               76   150     0       0    3      0
cpi_mean_tiled_kernel<2, true, true, true>                                  87   220     0       0    2      0
cpi_mean_tiled_kernel<2, true, true, false>                                 81   172     0       0    2      0
cpi_mean_tiled_kernel<2, false, true, true>                                 87   250     0       0    2      0
cpi_mean_tiled_kernel<2, false, true, false>                                81   175     0       0    2      0
cpi_mean_tiled_kernel<2, true, false, true>                                 82   220     0       0    2      0
cpi_mean_tiled_kernel<2, true, false, false>                                82   170     0       0    2      0
cpi_mean_tiled_kernel<2, false, false, true>                                82   250     0       0    2      0
cpi_mean_tiled_kernel<2, false, false, false>                               82   174     0       0    2      0
cpi_mean_running_kernel<2, false, true, true>                              104   234     0       0    1  36864
cpi_mean_running_kernel<2, false, true, false>                             102   222     0       0    1  36864
cpi_mean_running_kernel<2, false, false, true>                             104   234     0       0    1  36864
cpi_mean_running_kernel<2, false, false, false>                            102   222     0       0    1  36864
cpi_mean_running_kernel<1, true, true, true>                               106   256   106       0    1  36864
cpi_mean_running_kernel<1, true, true, false>                              106   256    94       0    1  36864
cpi_mean_running_kernel<1, true, false, true>                              106   256   104       0    1  36864
cpi_mean_running_kernel<1, true, false, false>                             106   256    94       0    1  36864
cpi_mean_running_kernel<1, false, true, true>                              104   216     0       0    1  36864
cpi_mean_running_kernel<1, false, true, false>                             102   206     0       0    1  36864
cpi_mean_running_kernel<1, false, false, true>                             104   216     0       0    1  36864
cpi_mean_running_kernel<1, false, false, false>                            102   206     0       0    1  36864
cpi_forster_kernel                                                          97   248     0       0    2  19200
cpi_cov_kernel<2, true>                                                    106   255     0       0    2  20096
cpi_cov_kernel<2, false>                                                   106   255     0       0    2  20096
cpi_cov_kernel<1, true>                                                    106   225     0       0    2  19904
cpi_cov_kernel<1, false>                                                   106   225     0       0    2  19904
cpi_cov_carry_kernel<2, true>                                              106   255     0       0    2  20096
cpi_cov_carry_kernel<2, false>                                             106   255     0       0    2  20096
cpi_cov_carry_kernel<1, true>                                              106   227     0       0    2  19904
cpi_cov_carry_kernel<1, false>                                             106   227     0       0    2  19904
cpi_cov_running_kernel<2, true>                                            106   255     0       0    2  20096
cpi_cov_running_kernel<2, false>                                           106   255     0       0    2  20096
cpi_cov_running_kernel<1, true>                                            106   230     0       0    2  19904
cpi_cov_running_kernel<1, false>                                           106   230     0       0    2  19904
cpi_unpack_slabs_kernel                                                     57    12     0       0    8      0
cpi_factor_kernel<1, true, 16, true>                                        56   139     0       0    3  11424
cpi_factor_kernel<1, true, 8, true>                                         51   156     0       0    2  30496
cpi_factor_kernel<1, true, 4, true>                                         58   256    80       0    1  60960
cpi_factor_kernel<2, true, 16, true>                                        58   148     0       0    3  11424
cpi_factor_kernel<2, true, 8, true>                                         58   154     0       0    2  30496
cpi_factor_kernel<2, true, 4, true>                                         58   256    82       0    1  60960
cpi_factor_kernel<1, true, 16, false>                                       56   139     0       0    3  11424
cpi_factor_kernel<1, true, 8, false>                                        51   164     0       0    1  37216
cpi_factor_kernel<1, true, 4, false>                                        58   256    56       0    1  74400
cpi_factor_kernel<2, true, 16, false>                                       58   148     0       0    3  11424
cpi_factor_kernel<2, true, 8, false>                                        58   164     0       0    1  37216
cpi_factor_kernel<2, true, 4, false>                                        58   256    60       0    1  74400
cpi_factor_kernel<1, false, 16, false>                                      48    90     0       0    4  11424
cpi_factor_kernel<1, false, 8, false>                                       44    96     0       0    2  22816
cpi_factor_kernel<1, false, 4, false>                                       44    92     0       0    1  45600
cpi_factor_kernel<2, false, 16, false>                                      58   120     0       0    4  11424
cpi_factor_kernel<2, false, 8, false>                                       58   128     0       0    2  22816
cpi_factor_kernel<2, false, 4, false>                                       58   112     0       0    1  45600
cpi_factor_packed_kernel<1, 2>                                              56   132     0       0    2  29696
cpi_factor_packed_kernel<1, 3>                                              52    87     0       0    2  19488
cpi_factor_packed_kernel<1, 4>                                              44    90     0       0    3  14848
cpi_factor_packed_kernel<1, 6>                                              46    90     0       0    5   9280
cpi_factor_packed_kernel<1, 8>                                              44    92     0       0    5   7424
cpi_factor_packed_kernel<2, 2>                                              56   158     0       0    2  29696
cpi_factor_packed_kernel<2, 3>                                              54   102     0       0    2  19488
cpi_factor_packed_kernel<2, 4>                                              50    98     0       0    3  14848
cpi_factor_packed_kernel<2, 6>                                              50    98     0       0    4   9280
cpi_factor_packed_kernel<2, 8>                                              45   100     0       0    4   7424
cpi_factor_hessian_kernel<1, true>                                          44   128     0      12    4   9792
cpi_factor_hessian_kernel<2, true>                                          46   128     0      12    4   9792
cpi_factor_hessian_kernel<1, false>                                         44   132     0       0    3  13152
cpi_factor_hessian_kernel<2, false>                                         46   132     0       0    3  13152
cpi_sqrt_info_kernel<true>                                                  43    70     0       0    7   3840
cpi_sqrt_info_kernel<false>                                                 26    70     0       0    6   7200
cpi_predict_kernel<1>                                                       43    94     0       0    3  13824
cpi_predict_kernel<2>                                                       36    94     0       0    3  13824
"""


@pytest.fixture(scope="module")
def lib():
    from cpi_amd import _lib
    return _lib.load()


def test_stream_running_symbols_are_declared_and_exported(lib):
    header = open(os.path.join(ROOT, "include", "cpi_amd.h")).read()
    from cpi_amd import build
    dyn = subprocess.run(["nm", "-D", "--defined-only", build.LIB], stdout=subprocess.PIPE, text=True, check=True).stdout
    additions = header.split("typedef struct cpi_ctx")[0].split("additions within 3")[1]
    for s in SYMBOLS:
        assert re.search(r"\bint %s\(" % s, header), s
        assert re.search(r" T %s$" % s, dyn, re.M), s
        assert getattr(lib, s).restype is C.c_int
        assert re.search(r"\b%s\b" % s, additions), s
    assert lib.cpi_abi_version() == 3
    # the "Not provided" sentences name the carry record only
    for path in (os.path.join(ROOT, "include", "cpi_amd.h"), os.path.join(ROOT, "INTEGRATION.md")):
        for sentence in re.findall(r"Not provided:[^\n]*(?:\n[^\n]*)?", open(path).read()):
            assert "stream entries" not in sentence, (path, sentence)


def test_stream_running_rejects_a_null_context(lib):
    from cpi_amd._lib import CpiOutputs, CpiParams
    prm, out = CpiParams(), CpiOutputs()
    assert lib.cpi_preintegrate_stream_running(None, C.byref(prm), 1, None, 1, None, 1, None, None, None, C.byref(out)) == 1
    assert lib.cpi_preintegrate_streams_running(None, C.byref(prm), 1, 1, None, None, 1, None, None, 1, None, None, None, C.byref(out)) == 1
    assert lib.cpi_preintegrate_stream_running_host(None, C.byref(prm), 1, None, 1, None, 1, None, None, C.byref(out), None) == 1
    assert lib.cpi_preintegrate_streams_running_host(None, C.byref(prm), 1, 1, None, None, 1, None, None, 1, None, None, C.byref(out), None) == 1


def test_engine_has_the_stream_running_entries():
    import inspect
    import cpi_amd
    for name in ("preintegrate_stream_running", "preintegrate_streams_running", "preintegrate_stream_running_host",
                 "preintegrate_streams_running_host"):
        fn = getattr(cpi_amd.Engine, name)
        assert callable(fn)
        par = inspect.signature(fn).parameters
        assert {"want", "N", "return_counts", "check_counts"} <= set(par), name
    for name in ("preintegrate_stream_running", "preintegrate_streams_running"):
        assert {"packed", "out", "workspace"} <= set(inspect.signature(getattr(cpi_amd.Engine, name)).parameters), name


def test_stream_running_kernels_are_in_the_resource_report_and_nothing_else_moved():
    from cpi_amd import build
    lines = open(build.REPORT).read().splitlines()
    new = [ln.split() for ln in lines if ln.startswith("cpi_mean_stream_running_kernel<")]
    names = " ".join(lines)
    for m in ("cpi_mean_stream_running_kernel<1, false, false, false>", "cpi_mean_stream_running_kernel<1, true, true, true>",
              "cpi_mean_stream_running_kernel<2, false, true, true>", "cpi_mean_stream_running_kernel<2, false, false, false>"):
        assert m in names, m
    assert "cpi_mean_stream_running_kernel<2, true" not in names   # model 2 has no running Jacobian kernel
    assert len(new) == 12 and all(r[-3] == "0" for r in new)       # scratch column
    norm = lambda ln: " ".join(ln.split())
    have = {norm(ln) for ln in lines}
    parent = [ln for ln in PARENT_ROWS.splitlines() if ln.strip()]
    assert len(parent) == 390
    missing = [ln for ln in parent if norm(ln) not in have]
    assert not missing, "rows of existing kernels changed: %s" % missing[:5]
    # and nothing but the new kernels was added
    assert len(lines) - 1 == len(parent) + len(new)
