// assembly.h -- the assembly handle of assembly.cpp for the other host files that work on one (vrs.cpp).
#pragma once

#include <cstdint>
#include <mutex>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/gtars_amd_host.h"
#include "seqstats.h"

struct gtars_assembly {
    std::vector<std::string> names;  // chromosome id -> name, ids in order of first appearance
    std::unordered_map<std::string, uint32_t> id;
    std::string blob;                // FASTA: the records' sequences back to back; .fab: the file
    std::vector<uint64_t> off, len;  // per chromosome id: its bytes in blob (the LAST record / entry of the name)
    std::mutex mu;                   // guards the lazy device image
    gtars::Assembly *dev = nullptr;
    std::mutex digest_mu;            // guards the lazy refget digests
    std::vector<char> refget;        // 33 bytes per chromosome: sha512t24u of its upper-cased bytes, NUL terminated
    bool refget_done = false;
    ~gtars_assembly() { gtars::assembly_free(dev); }
    void put(const std::string &name, uint64_t o, uint64_t l) {
        auto it = id.find(name);
        if (it == id.end()) {
            id.emplace(name, (uint32_t)names.size());
            names.push_back(name);
            off.push_back(o);
            len.push_back(l);
        } else {
            off[it->second] = o;
            len[it->second] = l;
        }
    }
};

namespace gtars {
// the handle's device image, built at the first call on the device current then
gtars_status assembly_device_image(gtars_assembly *a, Assembly **out);
}  // namespace gtars
