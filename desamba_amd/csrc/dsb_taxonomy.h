// Taxonomy and per-read records of the abundance report (internal; the public surface is include/desamba_amd.h).
#pragma once
#include <stdint.h>
#include <string>
#include <vector>
#include "../../include/desamba_amd.h"

#define DSB_TID_NONE 0xffffffffu      // parent of a taxid nodes.dmp does not list; also "odd reference name" in the device's table

struct dsb_taxonomy {
	uint32_t max_tid;                 // last line's taxid + 1 000 000 (the reference's table size)
	uint32_t *parent;                 // max_tid + 1 entries
	char (*rank)[20];
	uint32_t max_depth;               // longest chain of parent links (walks on the device are bounded by it)
	bool acyclic;                     // checked by dsb_taxonomy_load (dsb_taxonomy_load_any does not look)
	uint16_t *depth;                  // dsb_taxonomy_load only (else NULL): links from a rooted taxid to taxid 1, DSB_DEPTH_UNROOTED for the others
};
#define DSB_DEPTH_UNROOTED 0xffffu    // a taxid whose parent links do not reach taxid 1 (taxid 0 and unlisted taxids included)

// names.dmp: the "scientific name" of each taxid that has one, taxids ascending
struct dsb_taxnames { std::vector<uint32_t> tid; std::vector<std::string> name; };

// the taxid analysis reads from a reference name (the second '|' field, strtok rules); DSB_TID_NONE when the name would not
// come back from the SAM text as it is (empty, starting with '*', or holding a tab or a line end): the host walks those reads
uint32_t dsb_ref_taxid(const char *name);
// the walk of one read's own records (dsb_read_taxon.taxid), on the host: for the reads the device leaves to it
uint32_t dsb_read_taxid_host(const dsb_taxonomy *tx, const dsb_index *idx, uint32_t read_len, const dsb_hit *hits, uint32_t n, int max_sec_N);
