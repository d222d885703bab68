"""The f5c-side glue (integration/abea_glue.c) is a FILE a maintainer copies into f5c's src/; INTEGRATION.md quotes its two parts
verbatim, and this keeps the quotes and the file from drifting apart.  Compiling the glue against f5c's own headers and applying
integration/f5c_makefile.patch to f5c's Makefile need the f5c sources, which this repository does not hold."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_integration_md_quotes_the_glue_file():
    glue = open(os.path.join(ROOT, "integration", "abea_glue.c")).read()
    md = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    m = re.search(r"```c\n(// src/abea_glue\.c — .*?)```", md, re.S)
    assert m, "INTEGRATION.md lost its glue block"
    m2 = re.search(r"```c\n(// src/abea_glue\.c, continued.*?)```", md, re.S)      # the process_db_rsq chain (round 4)
    assert m2, "INTEGRATION.md lost its process_db_rsq glue block"
    assert m.group(1) in glue and m2.group(1) in glue, "INTEGRATION.md no longer quotes integration/abea_glue.c"


# The layout the shim's casts hand to f5c's structs, pinned as include/abea.h and include/abea_f5c_shim.h declare it (their comments
# cite the f5c.h lines each mirrors): a field moved, retyped or a constant changed in these headers fails here, not in a host build.
ABI = r'''
#include <stddef.h>
#include "abea_f5c_shim.h"
#ifdef __cplusplus
#define SA static_assert
#else
#define SA _Static_assert
#endif
#define OFF(t, f, v) SA(offsetof(t, f) == (v), #t "." #f)
SA(sizeof(abea_event_t) == 24, "abea_event_t");
OFF(abea_event_t, start, 0); OFF(abea_event_t, length, 8); OFF(abea_event_t, mean, 12); OFF(abea_event_t, stdv, 16);
SA(sizeof(abea_model_t) == 12, "abea_model_t");
OFF(abea_model_t, level_mean, 0); OFF(abea_model_t, level_stdv, 4); OFF(abea_model_t, level_log_stdv, 8);
SA(sizeof(abea_scalings_t) == 16, "abea_scalings_t");
OFF(abea_scalings_t, scale, 0); OFF(abea_scalings_t, shift, 4); OFF(abea_scalings_t, var, 8); OFF(abea_scalings_t, log_var, 12);
SA(sizeof(abea_pair_t) == 8, "abea_pair_t");
OFF(abea_pair_t, ref_pos, 0); OFF(abea_pair_t, read_pos, 4);
SA(sizeof(abea_index_pair_t) == 8, "abea_index_pair_t");
OFF(abea_index_pair_t, start, 0); OFF(abea_index_pair_t, stop, 4);
SA(sizeof(abea_f5c_event_table) == 4 * sizeof(void*), "abea_f5c_event_table");
OFF(abea_f5c_event_table, n, 0); OFF(abea_f5c_event_table, start, sizeof(size_t));
OFF(abea_f5c_event_table, end, 2 * sizeof(size_t)); OFF(abea_f5c_event_table, event, 3 * sizeof(size_t));
SA(ABEA_BANDWIDTH == 100 && ABEA_MAX_KMER_SIZE == 9, "compile-time constants");
SA(ABEA_FAILED_CALIBRATION == 0x001 && ABEA_FAILED_ALIGNMENT == 0x002 && ABEA_FAILED_QUALITY_CHK == 0x004,
               "read_stat_flag bits");
'''


def test_shim_abi_is_pinned(tmp_path):
    import subprocess
    src = tmp_path / "abi.c"
    src.write_text(ABI)
    for cmd in (["gcc", "-std=c11"], ["g++", "-x", "c++", "-std=c++11"]):          # f5c compiles its .c files as C++ on GPU builds
        r = subprocess.run(cmd + ["-fsyntax-only", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src)],
                           capture_output=True, text=True)
        assert r.returncode == 0, f"{cmd[0]}:\n{r.stderr[-3000:]}"
