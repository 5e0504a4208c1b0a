"""Every v18_* declaration of include/spangpu_spandsp.h against the reference's own src/spandsp/v18.h: a translation unit that
includes only the reference's headers initialises, for every name, a function pointer declared with our prototype's text from
the reference's function, under -Werror=incompatible-pointer-types."""
import os
import re

import pytest

from test_c_callers import REF, _prototypes, run

NAMES = {"v18_init", "v18_release", "v18_free", "v18_tx", "v18_rx", "v18_rx_fillin", "v18_put", "v18_get_current_mode",
         "v18_set_stored_message", "v18_mode_to_str", "v18_status_to_str", "v18_get_logging_state"}


def test_every_v18_name_is_declared(built):
    assert {p[0] for p in _prototypes("spangpu_spandsp.h", "SPANGPU_V18_API")} == NAMES
    # ... and is out of the way of the check over the fixed list of reference headers
    assert not NAMES & {p[0] for p in _prototypes("spangpu_spandsp.h", "SPANGPU_API")}


@pytest.mark.skipif(not os.path.isdir(REF), reason="the reference's headers are not here (GPU box)")
def test_v18_prototypes_are_the_references(built, tmp_path):
    ref_text = open(os.path.join(REF, "spandsp", "v18.h")).read()
    declared = set(re.findall(r"SPAN_DECLARE\([^)]*\)\s*(\w+)\s*\(", ref_text))
    assert declared == NAMES
    lines = ["#include <stdlib.h>", "#include <inttypes.h>", "#include <string.h>", "#include <stdio.h>", "#include <stdbool.h>"]
    for h in ("telephony", "logging", "async", "v18"):
        lines.append('#include "spandsp/%s.h"' % h)
    for name, ret, args in _prototypes("spangpu_spandsp.h", "SPANGPU_V18_API"):
        lines.append("static %s (*chk_%s)(%s) = %s;" % (ret, name, args, name))
    lines.append("int main(void) { return 0; }")
    src = os.path.join(str(tmp_path), "v18_proto_check.c")
    open(src, "w").write("\n".join(lines) + "\n")
    run(["gcc", "-std=gnu99", "-fsyntax-only", "-Wall", "-Werror", "-Werror=incompatible-pointer-types", "-Wno-unused-variable",
         "-DHAVE_STDBOOL_H", "-DHAVE_INTTYPES_H", "-DHAVE_STDINT_H", "-I" + REF, src])
