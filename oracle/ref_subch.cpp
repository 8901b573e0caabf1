// oracle/ref_subch.cpp -- TEST INFRASTRUCTURE: the reference's own Subchannel record (dab-constants.h:164-198) asked for the bit rate and
// the size in capacity units it derives from a sub-channel's protection settings (Subchannel::bitrate / numCU, dab-constants.cpp:404-477).
// Built by oracle/Makefile into _ref/libwelle_ref_subch.so against the unmodified dab-constants.cpp; tests/refapi.py loads it.
#include "dab-constants.h"

static Subchannel record(int shortForm, int uepTableIndex, int eepProfileB, int eepLevel, int length)
{
    Subchannel s; s.length = length; s.protectionSettings.shortForm = shortForm != 0;
    s.protectionSettings.uepTableIndex = uepTableIndex;
    s.protectionSettings.eepProfile = eepProfileB ? EEPProtectionProfile::EEP_B : EEPProtectionProfile::EEP_A;
    s.protectionSettings.eepLevel = (EEPProtectionLevel)eepLevel;
    return s;
}

extern "C" {

int ref_subch_bitrate_of(int shortForm, int uepTableIndex, int eepProfileB, int eepLevel, int length)
{
    return record(shortForm, uepTableIndex, eepProfileB, eepLevel, length).bitrate();
}

// (for the long form numCU goes through bitrate(), i.e. through `length`)
int ref_subch_num_cu(int shortForm, int uepTableIndex, int eepProfileB, int eepLevel, int length)
{
    return record(shortForm, uepTableIndex, eepProfileB, eepLevel, length).numCU();
}

}
