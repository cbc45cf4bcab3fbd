// The hashers of the library, one row each: what the validation (context.hip), the tree driver (path.hip) and the nonce
// search (grind.hip) need to know of a hasher id without launching anything.  No HIP in this header.  The kernels that go
// with a row are named once more, in dispatch_hasher (hasher_dispatch.hpp).
#pragma once
#include <stdint.h>

#include "../../include/wf_lde.h"
#include "grind_plan.hpp"
#include "merkle_plan.hpp"

namespace wf {

struct HasherRow {
    uint32_t id;       // enum wf_hasher
    const char *name;  // as error messages spell it
    bool digest24;     // a 24-byte digest exists (Blake3_192); every hasher has the 32-byte one
    bool f64_only;     // an element-digest hasher: it hashes elements of the f64 field only
    MerklePlan merkle;
    GrindPlan grind;
};

constexpr HasherRow HASHERS[] = {
    {WF_HASH_BLAKE3, "BLAKE3", true, false, MERKLE_PLAN_BLAKE3, GRIND_PLAN_BLAKE3},
    {WF_HASH_SHA3_256, "Sha3_256", false, false, MERKLE_PLAN_SHA3, GRIND_PLAN_SHA3},
    {WF_HASH_RP64_256, "Rp64_256", false, true, MERKLE_PLAN_RP64, GRIND_PLAN_RP64},
    {WF_HASH_RPJIVE64_256, "RpJive64_256", false, true, MERKLE_PLAN_RPJIVE, GRIND_PLAN_RPJIVE},
    {WF_HASH_GRIFFINJIVE64_256, "GriffinJive64_256", false, true, MERKLE_PLAN_GRIFFIN, GRIND_PLAN_GRIFFIN},
};

// the row of a hasher id; nullptr: no such hasher
inline const HasherRow *hasher_row(uint32_t id) {
    for (const HasherRow &r : HASHERS)
        if (r.id == id) return &r;
    return nullptr;
}

}  // namespace wf
