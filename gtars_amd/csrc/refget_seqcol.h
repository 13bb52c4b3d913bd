// refget_seqcol.h -- the sequence-collection handle of refget.cpp for the other host files that work on one (refget_pack.cpp).
#pragma once

#include <vector>

#include "assembly.h"
#include "refget_core.h"

// The records of one FASTA text in file order (a repeated name stays a record of its own).  With the bytes kept, `a` is an
// assembly over them with ONE entry per record -- its name map knows the last record of a name -- whose lazy device image
// serves the substring calls.
struct gtars_seqcol {
    std::vector<gtars::RefgetRecord> recs;
    std::vector<gtars::RefgetDigest> digests;  // per record, once computed
    bool has_digests = false, has_bytes = false, gzip = false;
    gtars::RefgetColDigests col;
    gtars_assembly a;
};
