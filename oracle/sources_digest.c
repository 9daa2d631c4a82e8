/* TEST INFRASTRUCTURE ONLY (see oracle.h): which sources this library was compiled from. oracle/Makefile passes the SHA-1 of all
 * the .c and .h files of oracle/; oracle_py.lib() looks for the marker in the file before it loads it and rebuilds a library that was
 * made from other sources, whatever the files' time stamps say (a library carried over from another checkout is newer than the
 * sources it does not match). */
#include "oracle.h"

#ifndef ORACLE_SOURCES_DIGEST
#define ORACLE_SOURCES_DIGEST "unknown"
#endif

const char* oracle_sources_digest(void)
{
	return "oracle-sources-digest:" ORACLE_SOURCES_DIGEST;
}
